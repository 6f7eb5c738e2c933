// kernels_cells.hip -- the cell-list pair search of nbody_fof_labels, nbody_fof_groups, nbody_contacts and
// nbody_merge_contacts under NBODY_SEARCH_CELLS (include/nbody_hip.h, "pair search"), on the device (gfx950).  Compiled with
// -ffp-contract=off; the grid is cell_grid.h's, the metric is k_fof_link's pair_dist2, the union is fof_union.h's.  No
// floating-point atomics, and no lane ever waits for another lane, wave or workgroup.  Every kernel reads the handle's state
// and writes the call's scratch only.
//
//   k_cells_bounds   min and max of the live, gridded bodies' coordinates and their number: doubles mapped to integers of the
//                    same order, reduced over the wave with shuffles, then one integer atomicMin / atomicMax per wave and
//                    bound (exact, and the order of arrival cannot show)
//   (the host reads the seven words, draws the grid with make_grid and decides whether it is usable)
//   k_cells_keys     key[i] of every row (rows past the live count and ungridded bodies: all ones), row[i] = i
//   (rocprim::radix_sort_pairs, stable, on (key, row): the gridded bodies cell after cell, ascending row within a cell)
//   k_cells_gather   the positions in that order; the distinct keys counted from the boundary flags (an integer atomicAdd)
//   k_cells_link     one gridded body per lane in key order, so a wave's lanes share cells; cell_walk.h's half walk: each
//                    unordered candidate pair is evaluated once, from its earlier body.  Where r2 < B2 the lane unites the
//                    ORIGINAL indices (fof_union.h; the proof that stale reads are harmless is DESIGN 3.18's)
//   k_cells_nearest  the full walk, over all nine columns: the least r2 < R2 and among equal r2 the lowest ORIGINAL index -- a
//                    rule on (r2, index) alone, so the order in which cells are visited cannot show
//   k_cells_within   k_cells_nearest's walk for the neighbour lists of kernels_within.h: a pass that counts every body's
//                    neighbours with r2 < R2, and after the caller's integer scan a pass that writes their ORIGINAL indices
//   k_cells_knn      k_cells_nearest's walk for the lists of kernels_knn.h: every gridded body's at most k nearest among the bodies
//                    with r2 < R2, in (r2, ORIGINAL index) order, and how many it found
//   k_cells_pair_hist  k_cells_link's walk for the binned pair counts of kernels_paircount.h: every candidate pair once, its r2
//                    binned by bin_slot, counted in a block-private LDS histogram that is added to the call's 64-bit slots
// The walks count their candidate pairs (place t after place s) in integers: shuffles, then one atomicAdd per wave.
#include "kernels_cells.h"
#include "cell_walk.h"
#include "device_util.h"   // inf64, live_count, wave_add
#include "fof_union.h"
#include "kernels_paircount.h"   // bin_slot, hist_begin, hist_flush
#include "kernels_knn.h"   // list_slots
#include "knn_list.h"
#include "real.h"      // widen
#include "scratch_carve.h"

#include <rocprim/device/device_radix_sort.hpp>


namespace nbody {

using pairs::kPairBlock;
using cells::cell_walk;
using cells::Walk;

namespace {

// a double as an integer of the same order (-0.0 below +0.0), and back
__host__ __device__ inline unsigned long long ordered_of(double v) {
    unsigned long long u;
    __builtin_memcpy(&u, &v, sizeof(u));
    return (u >> 63) ? ~u : u | (1ull << 63);
}
inline double double_of(unsigned long long o) {
    const unsigned long long u = (o >> 63) ? o & ~(1ull << 63) : ~o;
    double v;
    __builtin_memcpy(&v, &u, sizeof(v));
    return v;
}

}  // namespace

template <class F>
__global__ __launch_bounds__(kPairBlock) void k_cells_bounds(const typename Real<F>::V4* __restrict__ pos, const int* __restrict__ count,
                                                             int n_upper, cells::BoundsWords* out) {
    const int i = blockIdx.x * kPairBlock + threadIdx.x;
    unsigned long long lo[3] = {~0ull, ~0ull, ~0ull}, hi[3] = {0ull, 0ull, 0ull}, g = 0;
    if (i < live_count(count, n_upper)) {
        const double4 p = widen(pos[i]);
        if (cells::gridded(p.x, p.y, p.z)) {
            g = 1;
            lo[0] = hi[0] = ordered_of(p.x);
            lo[1] = hi[1] = ordered_of(p.y);
            lo[2] = hi[2] = ordered_of(p.z);
        }
    }
    for (int off = 32; off >= 1; off >>= 1) {   // (every lane of the wave is here)
        for (int c = 0; c < 3; ++c) {
            const unsigned long long l = __shfl_xor(lo[c], off, 64), h = __shfl_xor(hi[c], off, 64);
            lo[c] = l < lo[c] ? l : lo[c];
            hi[c] = h > hi[c] ? h : hi[c];
        }
        g += __shfl_xor(g, off, 64);
    }
    if (threadIdx.x % 64 == 0 && g) {
        for (int c = 0; c < 3; ++c) {
            atomicMin(&out->lo[c], lo[c]);
            atomicMax(&out->hi[c], hi[c]);
        }
        atomicAdd(&out->gridded, g);
    }
}

template <class F>
__global__ __launch_bounds__(kPairBlock) void k_cells_keys(const typename Real<F>::V4* __restrict__ pos, const int* __restrict__ count,
                                                           int n_upper, cells::Grid g, uint64_t* __restrict__ keys, int* __restrict__ rows) {
    const int i = blockIdx.x * kPairBlock + threadIdx.x;
    if (i >= n_upper) return;
    uint64_t key = cells::kNoKey;
    if (i < live_count(count, n_upper)) {
        const double4 p = widen(pos[i]);
        key = cells::body_key(g, p.x, p.y, p.z);
    }
    keys[i] = key;
    rows[i] = i;
}

// (the n_gridded keys that are not all ones stand first after the sort)
template <class F>
__global__ __launch_bounds__(kPairBlock) void k_cells_gather(const typename Real<F>::V4* __restrict__ pos, int n_gridded,
                                                             const uint64_t* __restrict__ keys, const int* __restrict__ rows,
                                                             double4* __restrict__ spos, cells::Counters* counters) {
    const int s = blockIdx.x * kPairBlock + threadIdx.x;
    unsigned long long head = 0;
    if (s < n_gridded) {
        spos[s] = widen(pos[rows[s]]);   // (rows[s] < the live count <= n_upper)
        head = s == 0 || keys[s] != keys[s - 1];
    }
    wave_add(head, &counters->occupied);
}

__global__ __launch_bounds__(kPairBlock) void k_cells_link(int n_gridded, const uint64_t* __restrict__ keys, const int* __restrict__ rows,
                                                           const double4* __restrict__ spos, double B2, int* parent,
                                                           cells::Counters* counters) {
    const int s = blockIdx.x * kPairBlock + threadIdx.x;
    unsigned long long cand = 0;
    if (s < n_gridded) {
        const double4 pi = spos[s];
        const int i = rows[s];
        const fof::DevParent forest{parent};
        cand = cell_walk<Walk::half>(keys, n_gridded, s, [&](int t) {
            const double r2 = fof::pair_dist2(pi, spos[t]);
            if (r2 < B2) fof::fof_link(forest, i, rows[t]);   // (strict; a NaN never links)
        });
    }
    wave_add(cand, &counters->candidates);
}

__global__ __launch_bounds__(kPairBlock) void k_cells_nearest_init(int n_upper, int* __restrict__ partner, double* __restrict__ energy) {
    const int i = blockIdx.x * kPairBlock + threadIdx.x;
    if (i >= n_upper) return;
    partner[i] = -1;
    energy[i] = inf64();
}

__global__ __launch_bounds__(kPairBlock) void k_cells_nearest(int n_gridded, const uint64_t* __restrict__ keys, const int* __restrict__ rows,
                                                              const double4* __restrict__ spos, double R2, int* __restrict__ partner,
                                                              double* __restrict__ energy, cells::Counters* counters) {
    const int s = blockIdx.x * kPairBlock + threadIdx.x;
    unsigned long long cand = 0;
    if (s < n_gridded) {
        const double4 pi = spos[s];
        double best = inf64();
        int best_j = -1;
        cand = cell_walk<Walk::full>(keys, n_gridded, s, [&](int t) {
            const double r2 = fof::pair_dist2(pi, spos[t]);
            if (!(r2 < R2)) return;   // (strict; a NaN is never within R)
            const int j = rows[t];
            if (r2 < best || (r2 == best && j < best_j)) { best = r2; best_j = j; }
        });
        partner[rows[s]] = best_j;
        energy[rows[s]] = best;
    }
    wave_add(cand, &counters->candidates);
}

// kFill == false: found[rows[s]] = the t != s of the nine columns with r2 < R2, their sum in 64 bits, and the candidate pairs as
// k_cells_nearest counts them.  kFill == true: the same walk again, the ORIGINAL indices written at offset[rows[s]] on, in the
// order of the walk (cells::launch_within_fill's caller sorts each list afterwards: integers, one result)
template <bool kFill>
__global__ __launch_bounds__(kPairBlock) void k_cells_within(int n_gridded, const uint64_t* __restrict__ keys, const int* __restrict__ rows,
                                                             const double4* __restrict__ spos, double R2, int* __restrict__ found,
                                                             const int* __restrict__ offset, int* __restrict__ raw, unsigned cap,
                                                             unsigned long long* total, cells::Counters* counters) {
    const int s = blockIdx.x * kPairBlock + threadIdx.x;
    unsigned long long cand = 0, hits = 0;
    if (s < n_gridded) {
        const double4 pi = spos[s];
        unsigned at = kFill ? unsigned(offset[rows[s]]) : 0u;
        cand = cell_walk<Walk::full>(keys, n_gridded, s, [&](int t) {
            const double r2 = fof::pair_dist2(pi, spos[t]);
            if (!(r2 < R2)) return;   // (strict; a NaN is never within R)
            if constexpr (kFill) {
                if (at < cap) raw[at] = rows[t];   // (at < cap always: the count pass saw the same state)
                ++at;
            } else {
                ++hits;
            }
        });
        if constexpr (!kFill) found[rows[s]] = int(hits);
    }
    if constexpr (!kFill) {   // (kFill: total and counters are null, and the walk's count is dropped)
        wave_add(hits, total);
        wave_add(cand, &counters->candidates);
    }
}

// k_cells_within's walk for the lists of kernels_knn.h: the at most k bodies t != s of the nine columns with r2 < R2 that come
// first in (r2, ORIGINAL index), kept in the lane's LDS list (knn_list.h) -- a rule on (r2, index) alone, so the order in which
// the cells are visited cannot show --, written as row rows[s]'s k {index, r2} padded with {-1, +inf}; found[rows[s]] = how
// many; the candidate pairs as k_cells_nearest counts them.  The last entry of a full list stands in registers: a candidate that
// does not come before it costs two compares.
template <int kSlots>
__global__ __launch_bounds__(kPairBlock) void k_cells_knn(int n_gridded, const uint64_t* __restrict__ keys, const int* __restrict__ rows,
                                                          const double4* __restrict__ spos, double R2, int k, int* __restrict__ found,
                                                          int* __restrict__ neighbor, double* __restrict__ dist2,
                                                          cells::Counters* counters) {
    __shared__ knn::ListLds<kSlots> lists;
    const int tid = threadIdx.x;
    const int s = blockIdx.x * kPairBlock + tid;
    unsigned long long cand = 0;
    if (s < n_gridded) {
        const double4 pi = spos[s];
        knn::ListState st;
        cand = cell_walk<Walk::full>(keys, n_gridded, s, [&](int t) {
            const double r2 = fof::pair_dist2(pi, spos[t]);
            if (!(r2 < R2)) return;   // (strict; a NaN is never within R)
            const int j = rows[t];
            if (st.admits(r2, j)) knn::list_insert(lists, tid, k, st, r2, j);
        });
        const size_t row = size_t(rows[s]);   // (< the live count <= n_upper)
        found[row] = st.held;
        for (int slot = 0; slot < k; ++slot) {
            neighbor[row * size_t(k) + size_t(slot)] = slot < st.held ? lists.j[slot][tid] : -1;
            dist2[row * size_t(k) + size_t(slot)] = slot < st.held ? lists.r2[slot][tid] : inf64();
        }
    }
    wave_add(cand, &counters->candidates);
}

// The binned pair counts of kernels_paircount.h over k_cells_link's walk: every candidate pair is evaluated once, from its
// earlier place (the body with the lower original row of the two when they share a cell), and counted in the slot of its r2 --
// but for the last slot: the pairs with !(r2 < E2[n_bins]) are not all candidates, so the caller obtains their number by
// subtraction.  A lane's first lane_budget counts go to the block's LDS words, any further one straight to the 64-bit slots
// (kernels_paircount.h: the overflow bound); the block adds its words at its end.
__global__ __launch_bounds__(kPairBlock) void k_cells_pair_hist(int n_gridded, const uint64_t* __restrict__ keys,
                                                                const double4* __restrict__ spos, const double* __restrict__ e2_global,
                                                                int n_bins, int top, unsigned lane_budget, unsigned long long* out,
                                                                cells::Counters* counters) {
    __shared__ double e2[paircount::kMaxBins + 1];
    __shared__ unsigned hist[paircount::kSlots];
    paircount::hist_begin(e2_global, n_bins, e2, hist);
    __syncthreads();
    const int s = blockIdx.x * kPairBlock + threadIdx.x;
    unsigned long long cand = 0;
    if (s < n_gridded) {
        const double4 pi = spos[s];
        unsigned used = 0;
        cand = cell_walk<Walk::half>(keys, n_gridded, s, [&](int t) {
            const int slot = paircount::bin_slot(e2, n_bins, top, fof::pair_dist2(pi, spos[t]));
            if (slot > n_bins) return;   // (beyond the last edge, or a NaN: counted by subtraction)
            if (used < lane_budget) {
                atomicAdd(hist + slot, 1u);
                ++used;
            } else {
                atomicAdd(out + slot, 1ull);
            }
        });
    }
    paircount::hist_flush(hist, n_bins, out);
    wave_add(cand, &counters->candidates);
}

namespace cells {

size_t bounds_of(const BoundsWords& w, double lo[3], double hi[3]) {
    for (int c = 0; c < 3; ++c) {
        lo[c] = w.gridded ? double_of(w.lo[c]) : 0.0;
        hi[c] = w.gridded ? double_of(w.hi[c]) : 0.0;
    }
    return size_t(w.gridded);
}

namespace {
size_t sort_tmp_bytes(size_t n_upper) {
    size_t b = 0;
    uint64_t* k = nullptr;
    int* v = nullptr;
    (void)rocprim::radix_sort_pairs(nullptr, b, k, k, v, v, n_upper, 0, 64, 0);
    return b;
}
CellScratch layout(Carver& c, size_t n_upper) {
    CellScratch w;
    w.counters = c.take<Counters>(1);
    w.keys = c.take<uint64_t>(2 * n_upper);
    w.rows = c.take<int>(2 * n_upper);
    w.spos = c.take<double4>(n_upper);
    w.sort_bytes = sort_tmp_bytes(n_upper);
    w.sort_tmp = c.take<char>(w.sort_bytes);
    return w;
}
}  // namespace

size_t scratch_bytes(size_t n_upper) { Carver c; layout(c, n_upper); return c.offset(); }
CellScratch scratch_layout(void* base, size_t n_upper) { Carver c(base); return layout(c, n_upper); }

template <class F>
void launch_bounds(hipStream_t s, const ShardT<F>& sh, int n_upper, BoundsWords* bounds) {
    (void)hipMemsetAsync(bounds, 0, sizeof(BoundsWords), s);
    (void)hipMemsetAsync(bounds->lo, 0xff, sizeof(bounds->lo), s);   // (a device address: nothing is read here)
    if (n_upper <= 0) return;
    hipLaunchKernelGGL(k_cells_bounds<F>, dim3(pairs::blocks_for(n_upper)), dim3(kPairBlock), 0, s, sh.own_pos(), sh.own_count(), n_upper,
                       bounds);
}

template <class F>
int launch_order(hipStream_t s, const ShardT<F>& sh, int n_upper, int n_gridded, const Grid& g, const CellScratch& w) {
    (void)hipMemsetAsync(w.counters, 0, sizeof(Counters), s);
    if (n_upper <= 0) return 0;
    hipLaunchKernelGGL(k_cells_keys<F>, dim3(pairs::blocks_for(n_upper)), dim3(kPairBlock), 0, s, sh.own_pos(), sh.own_count(), n_upper, g,
                       w.keys, w.rows);
    size_t tb = w.sort_bytes;
    if (rocprim::radix_sort_pairs(w.sort_tmp, tb, w.keys, w.keys + n_upper, w.rows, w.rows + n_upper, size_t(n_upper), 0, 64, s) != hipSuccess)
        return -1;
    if (n_gridded > 0)
        hipLaunchKernelGGL(k_cells_gather<F>, dim3(pairs::blocks_for(n_gridded)), dim3(kPairBlock), 0, s, sh.own_pos(), n_gridded,
                           w.sorted_keys(size_t(n_upper)), w.sorted_rows(size_t(n_upper)), w.spos, w.counters);
    return 0;
}

void launch_link_components(hipStream_t s, const int* live_count, int n_upper, int n_gridded, double B2, const CellScratch& w,
                            const fof::FofScratch& f) {
    if (n_upper <= 0) return;
    fof::launch_forest_init(s, live_count, n_upper, f);
    if (n_gridded > 0)
        hipLaunchKernelGGL(k_cells_link, dim3(pairs::blocks_for(n_gridded)), dim3(kPairBlock), 0, s, n_gridded, w.sorted_keys(size_t(n_upper)),
                           w.sorted_rows(size_t(n_upper)), w.spos, B2, f.parent, w.counters);
    fof::launch_flatten(s, live_count, n_upper, f);
}

void launch_nearest_within(hipStream_t s, int n_upper, int n_gridded, double R2, const CellScratch& w, const pairs::PairScratch& p) {
    if (n_upper <= 0) return;
    hipLaunchKernelGGL(k_cells_nearest_init, dim3(pairs::blocks_for(n_upper)), dim3(kPairBlock), 0, s, n_upper, p.partner, p.energy);
    if (n_gridded > 0)
        hipLaunchKernelGGL(k_cells_nearest, dim3(pairs::blocks_for(n_gridded)), dim3(kPairBlock), 0, s, n_gridded,
                           w.sorted_keys(size_t(n_upper)), w.sorted_rows(size_t(n_upper)), w.spos, R2, p.partner, p.energy, w.counters);
}

void launch_within_count(hipStream_t s, int n_upper, int n_gridded, double R2, const CellScratch& w, int* found, unsigned long long* total) {
    if (n_upper <= 0 || n_gridded <= 0) return;
    hipLaunchKernelGGL(k_cells_within<false>, dim3(pairs::blocks_for(n_gridded)), dim3(kPairBlock), 0, s, n_gridded,
                       w.sorted_keys(size_t(n_upper)), w.sorted_rows(size_t(n_upper)), w.spos, R2, found, static_cast<const int*>(nullptr),
                       static_cast<int*>(nullptr), 0u, total, w.counters);
}

void launch_within_fill(hipStream_t s, int n_upper, int n_gridded, double R2, const CellScratch& w, const int* offset, int* raw, size_t cap) {
    if (n_upper <= 0 || n_gridded <= 0 || !cap) return;
    hipLaunchKernelGGL(k_cells_within<true>, dim3(pairs::blocks_for(n_gridded)), dim3(kPairBlock), 0, s, n_gridded,
                       w.sorted_keys(size_t(n_upper)), w.sorted_rows(size_t(n_upper)), w.spos, R2, static_cast<int*>(nullptr), offset, raw,
                       unsigned(cap), static_cast<unsigned long long*>(nullptr), static_cast<Counters*>(nullptr));
}

void launch_knn(hipStream_t s, int n_upper, int n_gridded, int k, double R2, const CellScratch& w, int* found, int* neighbor, double* dist2) {
    if (n_upper <= 0 || k < 1 || k > knn::kSlotsLarge) return;
    (void)hipMemsetAsync(found, 0, size_t(n_upper) * sizeof(int), s);
    if (n_gridded <= 0) return;
    const dim3 grid(pairs::blocks_for(n_gridded)), block(kPairBlock);
    if (knn::list_slots(k) == knn::kSlotsSmall)
        hipLaunchKernelGGL(k_cells_knn<knn::kSlotsSmall>, grid, block, 0, s, n_gridded, w.sorted_keys(size_t(n_upper)),
                           w.sorted_rows(size_t(n_upper)), w.spos, R2, k, found, neighbor, dist2, w.counters);
    else
        hipLaunchKernelGGL(k_cells_knn<knn::kSlotsLarge>, grid, block, 0, s, n_gridded, w.sorted_keys(size_t(n_upper)),
                           w.sorted_rows(size_t(n_upper)), w.spos, R2, k, found, neighbor, dist2, w.counters);
}

void launch_pair_hist(hipStream_t s, int n_upper, int n_gridded, const CellScratch& w, const double* e2, int n_bins, int flush_tiles,
                      unsigned long long* hist) {
    if (n_upper <= 0 || n_gridded <= 0) return;
    hipLaunchKernelGGL(k_cells_pair_hist, dim3(pairs::blocks_for(n_gridded)), dim3(kPairBlock), 0, s, n_gridded,
                       w.sorted_keys(size_t(n_upper)), w.spos, e2, n_bins, paircount::search_top(n_bins),
                       unsigned(flush_tiles) * unsigned(kPairBlock), hist, w.counters);
}

template void launch_bounds<float>(hipStream_t, const ShardT<float>&, int, BoundsWords*);
template void launch_bounds<double>(hipStream_t, const ShardT<double>&, int, BoundsWords*);
template int launch_order<float>(hipStream_t, const ShardT<float>&, int, int, const Grid&, const CellScratch&);
template int launch_order<double>(hipStream_t, const ShardT<double>&, int, int, const Grid&, const CellScratch&);

}}  // namespace nbody::cells
