// kernels_paircount.hip -- the binned pair-separation counts of nbody_pair_counts and nbody_pair_counts_at
// (include/nbody_hip.h, "pair-separation counts") over all pairs, on the device (gfx950), f64 on either dtype.  Compiled with
// -ffp-contract=off (every product, sum and difference rounded on its own).  The result is integers only; no floating-point
// atomics.  The kernel reads the handle's state and writes the call's scratch only.
//
//   k_pair_hist   the all-pairs pass on k_partner's frame: one body per lane (its position in registers as doubles), the
//                 partners of a slice staged through LDS in tiles of 256, the grid (groups of 256 bodies) x K slices.
//                 kCross == false: the partners are the bodies themselves, r2_ij == r2_ji bit for bit, so only j > i is
//                 counted, a block whose whole partner range lies at or below its own bodies returns at once and the tiles
//                 below its first row are skipped, not masked (k_fof_link's rule): N^2 / 2 pair terms.
//                 kCross == true: the partners are the caller's points ({x, y, z} as doubles), d = point - body, every
//                 (body, point) pair counts.
//                 The squared edges stand in LDS; the slot of a pair is bin_slot's branch-free search; the count goes to the
//                 block's LDS word of 32 bits with an LDS integer atomic (kCombine: the lanes of a wave that hit one slot at
//                 the same partner first add up their number with ballots, kernels_paircount.h hist_add), and the block adds
//                 its words to the call's 64-bit slots after every flush_tiles tiles and at its end (hist_flush; the bound is
//                 in kernels_paircount.h).
#include "kernels_paircount.h"
#include "kernels.h"       // nbody::tuning()
#include "kernels_fof.h"   // pair_dist2
#include "pair_tiles.h"
#include "real.h"          // widen
#include "scratch_carve.h"

#include <algorithm>
#include <climits>

namespace nbody {

using paircount::kMaxBins;
using paircount::kPairBlock;
using paircount::kSlots;

template <class F, bool kCross, int kCombine>
__global__ __launch_bounds__(kPairBlock) void k_pair_hist(const typename Real<F>::V4* __restrict__ pos, const int* __restrict__ count,
                                                          int n_upper, int groups, int K, const double* __restrict__ points, int m,
                                                          const double* __restrict__ e2_global, int n_bins, int top, int flush_tiles,
                                                          unsigned long long* out) {
    __shared__ double4 tx[kPairBlock];
    __shared__ double e2[kMaxBins + 1];
    __shared__ unsigned hist[kSlots];
    const int n = live_count(count, n_upper);
    pairs::PairFrame f(groups, K, kCross ? m : n);
    if (f.first >= n) return;   // (block-uniform: no live body)
    if constexpr (!kCross) {
        if (!f.triangle()) return;   // (block-uniform: no partner j > i for any of its bodies)
    }
    paircount::hist_begin(e2_global, n_bins, e2, hist);   // (the tile loop's first barrier stands between this and any use)
    const int i = f.first + int(threadIdx.x);
    const bool live = i < n;
    const int mine = !live ? INT_MAX : kCross ? -1 : i;   // the partners above `mine` count: none | all | j > i
    const double4 pi = live ? widen(pos[i]) : make_double4(0.0, 0.0, 0.0, 0.0);
    int tiles = 0;
    pairs::for_each_partner(
        f,
        [&](int slot, int j) {
            if constexpr (kCross) {
                const double* q = points + 3 * size_t(j);
                tx[slot] = make_double4(q[0], q[1], q[2], 0.0);
            } else {
                tx[slot] = widen(pos[j]);
            }
        },
        [&](int j, int t) {
            const double r2 = fof::pair_dist2(pi, tx[t]);
            const int slot = j > mine ? paircount::bin_slot(e2, n_bins, top, r2) : -1;
            paircount::hist_add<kCombine>(hist, slot);
        },
        [&] {
            if (++tiles == flush_tiles) {   // (block-uniform)
                paircount::hist_flush(hist, n_bins, out);
                tiles = 0;
            }
        });
    paircount::hist_flush(hist, n_bins, out);
}

namespace paircount {

HistPlan make_hist_plan() {
    const Tuning& t = nbody::tuning();
    HistPlan p;
    p.flush_tiles = t.pair_hist_flush > 0 ? std::min(t.pair_hist_flush, kFlushTilesMax) : kFlushTilesMax;
    p.combine = t.pair_hist_combine == kCombineFirst || t.pair_hist_combine == kCombineAll ? t.pair_hist_combine : kCombineNone;
    return p;
}

namespace {
HistScratch layout(Carver& c, int n_bins, size_t batch) {
    HistScratch w;
    w.e2 = c.take<double>(size_t(n_bins + 1));
    w.hist = c.take<unsigned long long>(size_t(n_bins + 2));
    if (batch) w.points = c.take<double>(batch * 3);
    return w;
}

template <class F, bool kCross>
void launch(hipStream_t s, const ShardT<F>& sh, int n_upper, int m, const PartnerPlan& p, const HistPlan& hp, int n_bins, const HistScratch& w) {
    const dim3 grid(unsigned(p.groups) * unsigned(p.K)), block(kPairBlock);
    const int top = search_top(n_bins);
#define NBODY_PAIR_HIST(C)                                                                                                        \
    hipLaunchKernelGGL((k_pair_hist<F, kCross, C>), grid, block, 0, s, sh.own_pos(), sh.own_count(), n_upper, p.groups, p.K, w.points, m, \
                       w.e2, n_bins, top, hp.flush_tiles, w.hist)
    if (hp.combine == kCombineAll) NBODY_PAIR_HIST(kCombineAll);
    else if (hp.combine == kCombineFirst) NBODY_PAIR_HIST(kCombineFirst);
    else NBODY_PAIR_HIST(kCombineNone);
#undef NBODY_PAIR_HIST
}
}  // namespace

size_t scratch_bytes(int n_bins, size_t batch) { Carver c; layout(c, n_bins, batch); return c.offset(); }
HistScratch scratch_layout(void* base, int n_bins, size_t batch) { Carver c(base); return layout(c, n_bins, batch); }

template <class F>
void launch_auto(hipStream_t s, const ShardT<F>& sh, int n_upper, const PartnerPlan& p, const HistPlan& hp, int n_bins, const HistScratch& w) {
    if (n_upper <= 1 || p.groups <= 0) return;
    launch<F, false>(s, sh, n_upper, 0, p, hp, n_bins, w);
}

template <class F>
void launch_cross(hipStream_t s, const ShardT<F>& sh, int n_upper, int m, const PartnerPlan& p, const HistPlan& hp, int n_bins,
                  const HistScratch& w) {
    if (n_upper <= 0 || m <= 0 || p.groups <= 0) return;
    launch<F, true>(s, sh, n_upper, m, p, hp, n_bins, w);
}

template void launch_auto<float>(hipStream_t, const ShardT<float>&, int, const PartnerPlan&, const HistPlan&, int, const HistScratch&);
template void launch_auto<double>(hipStream_t, const ShardT<double>&, int, const PartnerPlan&, const HistPlan&, int, const HistScratch&);
template void launch_cross<float>(hipStream_t, const ShardT<float>&, int, int, const PartnerPlan&, const HistPlan&, int, const HistScratch&);
template void launch_cross<double>(hipStream_t, const ShardT<double>&, int, int, const PartnerPlan&, const HistPlan&, int, const HistScratch&);

}}  // namespace nbody::paircount
