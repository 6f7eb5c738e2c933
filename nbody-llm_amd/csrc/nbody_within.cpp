// nbody_within.cpp -- nbody_neighbors_within, nbody_density and nbody_density_center (include/nbody_hip.h, "neighbours within a
// radius"): the scratch of a call, the launches of kernels_within.hip (or, under NBODY_SEARCH_CELLS, of kernels_cells.hip's
// passes over the grid), the copies of what the caller asked for and the host's share of the centre's sums (the blocks in
// ascending order).  All three calls build the same lists with the same code: count, scan, fill (and, over a grid, sort).
#include "nbody_within.h"
#include "nbody_cells.h"

#include <algorithm>
#include <limits>
#include <string>
#include <vector>

namespace nbody { namespace within {

namespace {

constexpr uint64_t kMaxTotal = 2147483647ull;   // 2^31 - 1: every device-side index and rocPRIM size stays inside 32 bits

// The lists of one call on the device.  After count(): live, total and c.count; after fill(): c.offset [n_upper + 1] and
// l.neighbor [total] (null when total == 0), enqueued on the handle's stream.
template <class F>
struct Lists {
    Lists(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, double radius, const char* call)
        : h(h), sh(sh), n_upper(n_upper), R2(radius * radius), radius(radius), call(call), counts(h->mem), lists(h->mem), search(h->mem) {}

    // the grid, when the handle asks for one and it can be drawn; the count pass; the call's first synchronisation and the
    // record behind nbody_pair_search_stats (n_upper > 0)
    int count() {
        plan = pairs::make_partner_plan(int(n_upper));
        int rc = cells::prepare<F>(h, sh, n_upper, radius, call, &search);
        if (rc) return rc;
        if (search.on) plan.K = 1;   // one count per body
        HIP_TRY(h, counts.alloc(count_scratch_bytes(n_upper, plan.K)));
        c = count_scratch_layout(counts.get(), n_upper, plan.K);
        launch_clear(h->stream, c);
        if (search.on) cells::launch_within_count(h->stream, int(n_upper), search.n_gridded, R2, search.w, c.count, c.total);
        else launch_count_pairs<F>(h->stream, sh, int(n_upper), plan, R2, c);
        unsigned long long found = 0;
        int n_live = 0;
        cells::Counters counted;
        const hipError_t launched = hipGetLastError();
        const hipError_t found_copy = hipMemcpyAsync(&found, c.total, sizeof(found), hipMemcpyDeviceToHost, h->stream);
        const hipError_t live_copy = hipMemcpyAsync(&n_live, sh.own_count(), sizeof(int), hipMemcpyDeviceToHost, h->stream);
        rc = cells::fetch_counters(h, search, &counted);   // and the synchronisation, whatever was enqueued
        HIP_TRY(h, launched);
        HIP_TRY(h, found_copy);
        HIP_TRY(h, live_copy);
        if (rc) return rc;
        cells::record(h, search, counted);
        live = std::min(size_t(std::max(n_live, 0)), n_upper);
        total = found;
        return NBODY_OK;
    }

    bool too_many() const { return total > kMaxTotal; }
    int refuse_total() const {
        return fail(h, NBODY_ERR_CAPACITY, std::string(call) + ": more than 2^31 - 1 neighbours in all (" + std::to_string(total) +
                                               "); use a smaller radius");
    }

    // the scan and -- want_lists -- the fill pass (and the sort of the lists a grid filled), enqueued; total <= kMaxTotal
    int fill(bool want_lists = true) {
        bool prim_failed = launch_places(h->stream, int(n_upper), plan.K, c) != 0;
        if (want_lists && total && !prim_failed) {
            HIP_TRY(h, lists.alloc(list_scratch_bytes(n_upper, size_t(total), search.on)));
            l = list_scratch_layout(lists.get(), n_upper, size_t(total), search.on);
            if (search.on) {
                cells::launch_within_fill(h->stream, int(n_upper), search.n_gridded, R2, search.w, c.offset, l.raw, size_t(total));
                prim_failed = launch_sort_lists(h->stream, int(n_upper), c, l, size_t(total)) != 0;
            } else {
                launch_fill_pairs<F>(h->stream, sh, int(n_upper), plan, R2, c, l, size_t(total));
            }
        }
        HIP_TRY(h, hipGetLastError());
        if (prim_failed) {
            (void)hipStreamSynchronize(h->stream);
            return fail(h, NBODY_ERR_HIP, std::string(call) + ": rocPRIM call failed");
        }
        return NBODY_OK;
    }

    NbodyHandle* h;
    const ShardT<F>& sh;
    size_t n_upper;
    double R2, radius;
    const char* call;
    ScratchDev counts, lists;
    cells::Search search;
    pairs::PartnerPlan plan;
    CountScratch c;
    ListScratch l;
    size_t live = 0;
    uint64_t total = 0;
};

// hs and the normalisation of a kernel for `radius`, every product rounded on its own
void kernel_constants(double radius, int kernel, double* hs, double* norm) {
    *hs = radius * 0.5;
    if (kernel == NBODY_KERNEL_CUBIC_SPLINE) *norm = 3.141592653589793 * ((*hs * *hs) * *hs);
    else *norm = 4.1887902047863905 * ((radius * radius) * radius);
}

}  // namespace

template <class F>
int neighbors(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, double radius, uint64_t* offset, size_t cap, int32_t* neighbor,
              size_t neighbor_cap, size_t* n_out, uint64_t* n_neighbors_out) {
    if (n_out) *n_out = 0;
    if (n_neighbors_out) *n_neighbors_out = 0;
    if (!n_upper) {
        if (offset) offset[0] = 0;
        return NBODY_OK;
    }
    Lists<F> lists(h, sh, n_upper, radius, "nbody_neighbors_within");
    int rc = lists.count();
    if (rc) return rc;
    const size_t n = lists.live;
    if (n_out) *n_out = n;
    if (n_neighbors_out) *n_neighbors_out = lists.total;
    if (lists.too_many()) return lists.refuse_total();
    if ((offset && cap < n) || (neighbor && neighbor_cap < lists.total))
        return fail(h, NBODY_ERR_CAPACITY, "nbody_neighbors_within: buffer too small");
    if (!offset && !(neighbor && lists.total)) return NBODY_OK;   // counts only
    rc = lists.fill(neighbor != nullptr);
    if (rc) return rc;
    // only the n + 1 offsets and the listed neighbours cross to the host (both pageable: the copies return once the data has
    // reached them); the offsets are widened here
    std::vector<int> narrow(offset ? n + 1 : 0);
    hipError_t e = hipSuccess;
    if (offset) e = hipMemcpyAsync(narrow.data(), lists.c.offset, (n + 1) * sizeof(int), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess && neighbor && lists.total)
        e = hipMemcpyAsync(neighbor, lists.l.neighbor, size_t(lists.total) * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream);
    const hipError_t e_sync = hipStreamSynchronize(h->stream);
    HIP_TRY(h, e);
    HIP_TRY(h, e_sync);
    for (size_t i = 0; i < narrow.size(); ++i) offset[i] = uint64_t(narrow[i]);   // (rows past the live count hold no neighbours: offset[n] = total)
    return NBODY_OK;
}
template int neighbors<float>(NbodyHandle*, const ShardT<float>&, size_t, double, uint64_t*, size_t, int32_t*, size_t, size_t*, uint64_t*);
template int neighbors<double>(NbodyHandle*, const ShardT<double>&, size_t, double, uint64_t*, size_t, int32_t*, size_t, size_t*, uint64_t*);

template <class F>
int density(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, double radius, int kernel, double* rho, int32_t* count, size_t cap,
            size_t* n_out) {
    if (n_out) *n_out = 0;
    if (!n_upper) return NBODY_OK;
    Lists<F> lists(h, sh, n_upper, radius, "nbody_density");
    int rc = lists.count();
    if (rc) return rc;
    const size_t n = lists.live;
    if (n_out) *n_out = n;
    if (lists.too_many()) return lists.refuse_total();
    if ((rho || count) && cap < n) return fail(h, NBODY_ERR_CAPACITY, "nbody_density: buffer too small");
    if ((!rho && !count) || !n) return NBODY_OK;
    rc = lists.fill();
    if (rc) return rc;
    ScratchDev out(h->mem);   // [n_upper] rho | [n_upper] count
    const size_t rho_bytes = (n_upper * sizeof(double) + 255) / 256 * 256;
    HIP_TRY(h, out.alloc(rho_bytes + n_upper * sizeof(int)));
    double* d_rho = out.get<double>();
    int* d_count = reinterpret_cast<int*>(out.get<char>() + rho_bytes);
    double hs, norm;
    kernel_constants(radius, kernel, &hs, &norm);
    launch_density<F>(h->stream, sh, int(n_upper), kernel == NBODY_KERNEL_CUBIC_SPLINE, hs, norm, lists.c.offset, lists.l.neighbor,
                      rho ? d_rho : nullptr, count ? d_count : nullptr);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && rho) e = hipMemcpyAsync(rho, d_rho, n * sizeof(double), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess && count) e = hipMemcpyAsync(count, d_count, n * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream);
    const hipError_t e_sync = hipStreamSynchronize(h->stream);
    HIP_TRY(h, e);
    HIP_TRY(h, e_sync);
    return NBODY_OK;
}
template int density<float>(NbodyHandle*, const ShardT<float>&, size_t, double, int, double*, int32_t*, size_t, size_t*);
template int density<double>(NbodyHandle*, const ShardT<double>&, size_t, double, int, double*, int32_t*, size_t, size_t*);

template <class F>
int center_sums(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, const double* d_rho, double sum[kCenterSums]) {
    for (int q = 0; q < kCenterSums; ++q) sum[q] = 0.0;
    if (!n_upper) return NBODY_OK;
    const size_t blocks = size_t(pairs::blocks_for(int(n_upper)));
    ScratchDev out(h->mem);   // [blocks][kCenterSums] block sums
    HIP_TRY(h, out.alloc(blocks * kCenterSums * sizeof(double)));
    double* d_part = out.get<double>();
    launch_center<F>(h->stream, sh, int(n_upper), d_rho, d_part);
    std::vector<double> part(blocks * kCenterSums);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(part.data(), d_part, part.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream);
    const hipError_t e_sync = hipStreamSynchronize(h->stream);
    HIP_TRY(h, e);
    HIP_TRY(h, e_sync);
    for (size_t b = 0; b < blocks; ++b)   // blocks in ascending order
        for (int q = 0; q < kCenterSums; ++q) sum[q] += part[b * kCenterSums + q];
    return NBODY_OK;
}
template int center_sums<float>(NbodyHandle*, const ShardT<float>&, size_t, const double*, double*);
template int center_sums<double>(NbodyHandle*, const ShardT<double>&, size_t, const double*, double*);

template <class F>
int density_center(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, double radius, int kernel, double center[3], double* rho_sum) {
    double sum[kCenterSums] = {0.0, 0.0, 0.0, 0.0};
    const auto finish = [&]() {
        for (int k = 0; k < 3; ++k) center[k] = sum[1 + k] / sum[0];   // (no bodies: 0 / 0)
        if (rho_sum) *rho_sum = sum[0];
        return NBODY_OK;
    };
    for (int k = 0; k < 3; ++k) center[k] = std::numeric_limits<double>::quiet_NaN();
    if (rho_sum) *rho_sum = 0.0;
    if (!n_upper) return finish();
    Lists<F> lists(h, sh, n_upper, radius, "nbody_density_center");
    int rc = lists.count();
    if (rc) return rc;
    if (lists.too_many()) return lists.refuse_total();
    if (!lists.live) return finish();
    rc = lists.fill();
    if (rc) return rc;
    ScratchDev out(h->mem);   // [n_upper] rho
    HIP_TRY(h, out.alloc(n_upper * sizeof(double)));
    double* d_rho = out.get<double>();
    double hs, norm;
    kernel_constants(radius, kernel, &hs, &norm);
    launch_density<F>(h->stream, sh, int(n_upper), kernel == NBODY_KERNEL_CUBIC_SPLINE, hs, norm, lists.c.offset, lists.l.neighbor, d_rho,
                      nullptr);
    rc = center_sums<F>(h, sh, n_upper, d_rho, sum);
    if (rc) return rc;
    return finish();
}
template int density_center<float>(NbodyHandle*, const ShardT<float>&, size_t, double, int, double*, double*);
template int density_center<double>(NbodyHandle*, const ShardT<double>&, size_t, double, int, double*, double*);

}}  // namespace nbody::within
