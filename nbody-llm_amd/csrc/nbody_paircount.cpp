// nbody_paircount.cpp -- nbody_pair_counts and nbody_pair_counts_at (include/nbody_hip.h, "pair-separation counts"): the
// squared edges, the scratch of a call, the launch of kernels_paircount.hip's all-pairs pass (or, under NBODY_SEARCH_CELLS, of
// kernels_cells.hip's pass over the grid), and the n_bins + 2 integers that cross to the host.
#include "nbody_paircount.h"
#include "nbody_cells.h"

#include <algorithm>
#include <cmath>

namespace nbody { namespace paircount {

namespace {

constexpr size_t kPointBatch = size_t(1) << 20;   // points of one launch of pair_counts_at (24 MiB of scratch; indices stay ints)

// counts and outside from the n_bins + 2 slots; over: what outside[1] is (the last slot, or the caller's subtraction)
void hand_out(const std::vector<unsigned long long>& slots, int n_bins, unsigned long long over, uint64_t* counts, uint64_t* outside) {
    for (int b = 0; b < n_bins; ++b) counts[b] = slots[size_t(b) + 1];
    if (outside) {
        outside[0] = slots[0];
        outside[1] = over;
    }
}

}  // namespace

std::string squared_edges(const double* edges, int n_bins, std::vector<double>* e2) {
    if (n_bins < 1 || n_bins > kMaxBins) return "n_bins must be in 1 .. NBODY_PAIR_COUNT_MAX_BINS (1024)";
    if (!edges) return "edges is NULL";
    e2->resize(size_t(n_bins) + 1);
    for (int b = 0; b <= n_bins; ++b) {
        if (!std::isfinite(edges[b])) return "edge " + std::to_string(b) + " is not finite";
        (*e2)[size_t(b)] = edges[b] * edges[b];   // rounded once
    }
    if (!(edges[0] >= 0.0)) return "edges[0] must be >= 0";
    for (int b = 0; b <= n_bins; ++b) {
        if (!std::isfinite((*e2)[size_t(b)])) return "the square of edge " + std::to_string(b) + " is not finite";
        if (b && !((*e2)[size_t(b) - 1] < (*e2)[size_t(b)]))
            return "the squares of the edges must strictly ascend (edge " + std::to_string(b) + ")";
    }
    return std::string();
}

template <class F>
int pair_counts(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, const std::vector<double>& e2, double length, uint64_t* counts,
                uint64_t* outside) {
    const int n_bins = int(e2.size()) - 1;
    std::vector<unsigned long long> slots(size_t(n_bins) + 2, 0);
    hand_out(slots, n_bins, 0, counts, outside);
    if (!n_upper) return NBODY_OK;
    const PartnerPlan plan = pairs::make_partner_plan(int(n_upper));
    const HistPlan hp = make_hist_plan();
    cells::Search search(h->mem);
    int rc = cells::prepare<F>(h, sh, n_upper, length, "nbody_pair_counts", &search);
    if (rc) return rc;
    ScratchDev scratch(h->mem);
    HIP_TRY(h, scratch.alloc(scratch_bytes(n_bins, 0)));
    const HistScratch w = scratch_layout(scratch.get(), n_bins, 0);
    // (e2 is pageable: the copy returns once the data has left it)
    HIP_TRY(h, hipMemcpyAsync(w.e2, e2.data(), e2.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemsetAsync(w.hist, 0, slots.size() * sizeof(unsigned long long), h->stream));
    if (search.on) cells::launch_pair_hist(h->stream, int(n_upper), search.n_gridded, search.w, w.e2, n_bins, hp.flush_tiles, w.hist);
    else launch_auto<F>(h->stream, sh, int(n_upper), plan, hp, n_bins, w);
    int n_live = 0;
    cells::Counters counted;
    const hipError_t launched = hipGetLastError();
    const hipError_t slots_copy = hipMemcpyAsync(slots.data(), w.hist, slots.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream);
    const hipError_t live_copy = hipMemcpyAsync(&n_live, sh.own_count(), sizeof(int), hipMemcpyDeviceToHost, h->stream);
    rc = cells::fetch_counters(h, search, &counted);   // and the synchronisation, whatever was enqueued
    HIP_TRY(h, launched);
    HIP_TRY(h, slots_copy);
    HIP_TRY(h, live_copy);
    if (rc) return rc;
    cells::record(h, search, counted);
    unsigned long long over = slots.back();
    if (search.on) {   // the pairs the walk never met stand beyond the last edge: n (n - 1) / 2 less everything it counted
        const unsigned long long n = std::min(size_t(std::max(n_live, 0)), n_upper);
        unsigned long long met = 0;
        for (int k = 0; k <= n_bins; ++k) met += slots[size_t(k)];
        over = n * (n ? n - 1 : 0) / 2 - met;
    }
    hand_out(slots, n_bins, over, counts, outside);
    return NBODY_OK;
}
template int pair_counts<float>(NbodyHandle*, const ShardT<float>&, size_t, const std::vector<double>&, double, uint64_t*, uint64_t*);
template int pair_counts<double>(NbodyHandle*, const ShardT<double>&, size_t, const std::vector<double>&, double, uint64_t*, uint64_t*);

template <class F>
int pair_counts_at(NbodyHandle* h, const ShardT<F>& sh, size_t n_upper, const double* points, size_t m, const std::vector<double>& e2,
                   uint64_t* counts, uint64_t* outside) {
    const int n_bins = int(e2.size()) - 1;
    std::vector<unsigned long long> slots(size_t(n_bins) + 2, 0);
    hand_out(slots, n_bins, 0, counts, outside);
    if (!n_upper || !m) return NBODY_OK;
    const size_t batch = std::min(m, kPointBatch);
    const HistPlan hp = make_hist_plan();
    ScratchDev scratch(h->mem);
    HIP_TRY(h, scratch.alloc(scratch_bytes(n_bins, batch)));
    const HistScratch w = scratch_layout(scratch.get(), n_bins, batch);
    HIP_TRY(h, hipMemcpyAsync(w.e2, e2.data(), e2.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemsetAsync(w.hist, 0, slots.size() * sizeof(unsigned long long), h->stream));
    for (size_t at = 0; at < m; at += batch) {
        const int mb = int(std::min(batch, m - at));
        const PartnerPlan plan = pairs::make_partner_plan(int(n_upper), mb);
        HIP_TRY(h, hipMemcpyAsync(w.points, points + 3 * at, size_t(mb) * 3 * sizeof(double), hipMemcpyHostToDevice, h->stream));
        launch_cross<F>(h->stream, sh, int(n_upper), mb, plan, hp, n_bins, w);
        HIP_TRY(h, hipGetLastError());
        if (at + batch < m) HIP_TRY(h, hipStreamSynchronize(h->stream));   // (the batch's points are overwritten by the next one)
    }
    const hipError_t slots_copy = hipMemcpyAsync(slots.data(), w.hist, slots.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream);
    const hipError_t stream_sync = hipStreamSynchronize(h->stream);   // whether or not the copy was enqueued: slots is a local
    HIP_TRY(h, slots_copy);
    HIP_TRY(h, stream_sync);
    hand_out(slots, n_bins, slots.back(), counts, outside);
    return NBODY_OK;
}
template int pair_counts_at<float>(NbodyHandle*, const ShardT<float>&, size_t, const double*, size_t, const std::vector<double>&, uint64_t*, uint64_t*);
template int pair_counts_at<double>(NbodyHandle*, const ShardT<double>&, size_t, const double*, size_t, const std::vector<double>&, uint64_t*, uint64_t*);

}}  // namespace nbody::paircount
