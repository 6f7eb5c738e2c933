// nbody_knn.cpp -- nbody_knn, nbody_knn_density and nbody_knn_density_center (include/nbody_hip.h, "k nearest neighbours"):
// the scratch of a call, the launches of kernels_knn.hip (and, under NBODY_SEARCH_CELLS with a hint, of kernels_cells.hip's
// k_cells_knn before them), the copies of what the caller asked for and, for the centre, nbody_within.cpp's sums.  All three
// calls build the same rows of k {index, r2} with the same code.
#include "nbody_knn.h"
#include "nbody_cells.h"
#include "nbody_within.h"   // center_sums

#include <algorithm>
#include <limits>
#include <string>

namespace nbody { namespace knn {

namespace {

// The rows of one call on the device.  After run(): live, answered[] and w.neighbor / w.dist2 [n_upper][k], enqueued on the
// handle's stream (n_upper > 0).
template <class F>
struct Rows {
    Rows(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, int k, double hint, const char* call)
        : h(h), sh(sh), n_upper(n_upper), k(k), hint(hint), call(call), scratch(h->mem), records(h->mem), search(h->mem) {}

    // one all-pairs pass: over every row (list == nullptr) or over the `rows` rows of the list
    int pairs_pass(const int* list, size_t rows) {
        const pairs::PartnerPlan plan = pairs::make_partner_plan(int(rows), int(n_upper));
        HIP_TRY(h, records.alloc(record_bytes(plan, k)));
        record_layout(records.get(), plan, k, &w);
        launch_pairs<F>(h->stream, sh, int(n_upper), k, list, int(rows), plan, w);
        HIP_TRY(h, hipGetLastError());
        return NBODY_OK;
    }

    int run() {
        int rc = hint > 0.0 ? cells::prepare<F>(h, sh, n_upper, hint, call, &search) : NBODY_OK;   // (no hint: search.on stays false)
        if (rc) return rc;
        HIP_TRY(h, scratch.alloc(scratch_bytes(n_upper, k, search.on)));
        w = scratch_layout(scratch.get(), n_upper, k, search.on);
        int n_live = 0;
        if (!search.on) {   // every row from the all-pairs pass; the record behind nbody_pair_search_stats stays as it was
            rc = pairs_pass(nullptr, n_upper);
            if (rc) return rc;
            const hipError_t live_copy = hipMemcpyAsync(&n_live, sh.own_count(), sizeof(int), hipMemcpyDeviceToHost, h->stream);
            const hipError_t e_sync = hipStreamSynchronize(h->stream);
            HIP_TRY(h, live_copy);
            HIP_TRY(h, e_sync);
            live = std::min(size_t(std::max(n_live, 0)), n_upper);
            answered[0] = 0;
            answered[1] = live;
            return NBODY_OK;
        }
        // the gridded rows from their 27 cells; the rows that found fewer than k there, and the rows that are not gridded, in a
        // list; the call's one read-back of how many; then exactly those rows from the all-pairs pass
        cells::launch_knn(h->stream, int(n_upper), search.n_gridded, k, hint * hint, search.w, w.found, w.neighbor, w.dist2);
        const bool scan_failed = launch_unfinished(h->stream, sh.own_count(), int(n_upper), k, w) != 0;
        int unfinished = 0;
        cells::Counters counted;
        const hipError_t launched = hipGetLastError();
        const hipError_t total_copy = scan_failed ? hipSuccess : hipMemcpyAsync(&unfinished, w.total, sizeof(int), hipMemcpyDeviceToHost, h->stream);
        const hipError_t live_copy = hipMemcpyAsync(&n_live, sh.own_count(), sizeof(int), hipMemcpyDeviceToHost, h->stream);
        rc = cells::fetch_counters(h, search, &counted);   // and the synchronisation, whatever was enqueued
        HIP_TRY(h, launched);
        HIP_TRY(h, total_copy);
        HIP_TRY(h, live_copy);
        if (rc) return rc;
        if (scan_failed) return fail(h, NBODY_ERR_HIP, std::string(call) + ": rocPRIM call failed");
        cells::record(h, search, counted);
        live = std::min(size_t(std::max(n_live, 0)), n_upper);
        const size_t m = std::min(size_t(std::max(unfinished, 0)), live);
        answered[0] = live - m;
        answered[1] = m;
        return m ? pairs_pass(w.list, m) : NBODY_OK;
    }

    NbodyHandle* h;
    const ShardT<F>& sh;
    size_t n_upper;
    int k;
    double hint;
    const char* call;
    ScratchDev scratch, records;
    cells::Search search;
    KnnScratch w;
    size_t live = 0;
    uint64_t answered[2] = {0, 0};   // rows answered from the cells, rows answered by the all-pairs pass
};

// the live count of sh alone, for a call that only counts
template <class F>
int count_only(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, size_t* n_out) {
    int live = 0;
    hipError_t e = hipMemcpyAsync(&live, sh.own_count(), sizeof(int), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    HIP_TRY(h, e);
    if (n_out) *n_out = std::min(size_t(std::max(live, 0)), n_upper);
    return NBODY_OK;
}

}  // namespace

template <class F>
int neighbors(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, int k, double radius_hint, int32_t* neighbor, double* dist2, size_t cap,
              size_t* n_out, uint64_t stats[2]) {
    if (n_out) *n_out = 0;
    if (stats) stats[0] = stats[1] = 0;
    if (!n_upper) return NBODY_OK;
    if (!neighbor && !dist2) return count_only<F>(h, sh, n_upper, n_out);
    Rows<F> rows(h, sh, n_upper, k, radius_hint, "nbody_knn");
    int rc = rows.run();
    if (rc) {
        (void)hipStreamSynchronize(h->stream);
        return rc;
    }
    const size_t n = rows.live;
    const bool fits = n <= cap;
    // (neighbor and dist2 are pageable: the copies return once the data has reached them)
    hipError_t e = hipSuccess;
    if (fits && n && neighbor) e = hipMemcpyAsync(neighbor, rows.w.neighbor, n * size_t(k) * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess && fits && n && dist2)
        e = hipMemcpyAsync(dist2, rows.w.dist2, n * size_t(k) * sizeof(double), hipMemcpyDeviceToHost, h->stream);
    const hipError_t e_sync = hipStreamSynchronize(h->stream);
    HIP_TRY(h, e);
    HIP_TRY(h, e_sync);
    if (n_out) *n_out = n;
    if (!fits) return fail(h, NBODY_ERR_CAPACITY, "nbody_knn: buffer too small");
    if (stats) { stats[0] = rows.answered[0]; stats[1] = rows.answered[1]; }
    return NBODY_OK;
}
template int neighbors<float>(NbodyHandle*, const ShardT<float>&, size_t, int, double, int32_t*, double*, size_t, size_t*, uint64_t*);
template int neighbors<double>(NbodyHandle*, const ShardT<double>&, size_t, int, double, int32_t*, double*, size_t, size_t*, uint64_t*);

template <class F>
int density(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, int k, double radius_hint, double* rho, double* rk2, size_t cap, size_t* n_out) {
    if (n_out) *n_out = 0;
    if (!n_upper) return NBODY_OK;
    if (!rho && !rk2) return count_only<F>(h, sh, n_upper, n_out);
    Rows<F> rows(h, sh, n_upper, k, radius_hint, "nbody_knn_density");
    int rc = rows.run();
    if (rc) {
        (void)hipStreamSynchronize(h->stream);
        return rc;
    }
    const size_t n = rows.live;
    if (n_out) *n_out = n;
    if (cap < n) {
        (void)hipStreamSynchronize(h->stream);
        return fail(h, NBODY_ERR_CAPACITY, "nbody_knn_density: buffer too small");
    }
    ScratchDev out(h->mem);   // [n_upper] rho | [n_upper] rk2
    const size_t rho_bytes = (n_upper * sizeof(double) + 255) / 256 * 256;
    HIP_TRY(h, out.alloc(2 * rho_bytes));
    double* d_rho = out.get<double>();
    double* d_rk2 = reinterpret_cast<double*>(out.get<char>() + rho_bytes);
    launch_density<F>(h->stream, sh, int(n_upper), k, rows.w, rho ? d_rho : nullptr, rk2 ? d_rk2 : nullptr);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && n && rho) e = hipMemcpyAsync(rho, d_rho, n * sizeof(double), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess && n && rk2) e = hipMemcpyAsync(rk2, d_rk2, n * sizeof(double), hipMemcpyDeviceToHost, h->stream);
    const hipError_t e_sync = hipStreamSynchronize(h->stream);
    HIP_TRY(h, e);
    HIP_TRY(h, e_sync);
    return NBODY_OK;
}
template int density<float>(NbodyHandle*, const ShardT<float>&, size_t, int, double, double*, double*, size_t, size_t*);
template int density<double>(NbodyHandle*, const ShardT<double>&, size_t, int, double, double*, double*, size_t, size_t*);

template <class F>
int density_center(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, int k, double radius_hint, double center[3], double* rho_sum) {
    double sum[within::kCenterSums] = {0.0, 0.0, 0.0, 0.0};
    const auto finish = [&]() {
        for (int c = 0; c < 3; ++c) center[c] = sum[1 + c] / sum[0];   // (no bodies, or no complete row: 0 / 0)
        if (rho_sum) *rho_sum = sum[0];
        return NBODY_OK;
    };
    for (int c = 0; c < 3; ++c) center[c] = std::numeric_limits<double>::quiet_NaN();
    if (rho_sum) *rho_sum = 0.0;
    if (!n_upper) return finish();
    Rows<F> rows(h, sh, n_upper, k, radius_hint, "nbody_knn_density_center");
    int rc = rows.run();
    if (rc) {
        (void)hipStreamSynchronize(h->stream);
        return rc;
    }
    if (!rows.live) {
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        return finish();
    }
    ScratchDev out(h->mem);   // [n_upper] rho
    HIP_TRY(h, out.alloc(n_upper * sizeof(double)));
    launch_density<F>(h->stream, sh, int(n_upper), k, rows.w, out.get<double>(), nullptr);
    rc = within::center_sums<F>(h, sh, n_upper, out.get<double>(), sum);
    if (rc) return rc;
    return finish();
}
template int density_center<float>(NbodyHandle*, const ShardT<float>&, size_t, int, double, double*, double*);
template int density_center<double>(NbodyHandle*, const ShardT<double>&, size_t, int, double, double*, double*);

}}  // namespace nbody::knn
