// kernels_knn.hip -- every body's exact k nearest neighbours (nbody_knn, nbody_knn_density, nbody_knn_density_center:
// include/nbody_hip.h, "k nearest neighbours"), on the device (gfx950), f64 on either dtype.  Compiled with -ffp-contract=off
// (every product, sum and difference rounded on its own; sqrt and divide are IEEE).  No floating-point atomics: the same state
// gives the same bits.  Every kernel reads the handle's state and writes the call's scratch only.
//
//   k_knn_pairs    the all-pairs pass on k_partner's frame: one row per lane, the partners of a slice staged through LDS in
//                  tiles of 256, j ascending; the grid is (groups of 256 rows) x K slices.  Each lane keeps the at most k
//                  best (r2, j) of its slice in an LDS list (knn_list.h), ascending in (r2, j); the r2 of the list's last
//                  entry -- +inf while the list is not full -- stands in a register, and a partner that fails r2 < that
//                  costs one compare.  j ascends within a slice, so a partner that ties with the last entry comes after it:
//                  the strict compare is the (r2, j) order.  kList: the rows are list[0 .. rows - 1] (the rows the cell pass
//                  left unfinished) instead of 0 .. live - 1.  The list of (slice, row place) goes to rec, padded
//   k_knn_merge    one row per lane: the K slice lists of the row in ascending slice order through the same LDS list under the
//                  same compare -- ascending slices hold ascending j, so the result is the list one slice over all partners
//                  would have kept, whatever K is -- written as the row's k {index, r2}, padded with {-1, +inf}
//   k_knn_flag     1 where a live row's cell pass kept fewer than k bodies (rows that are not gridded: 0 kept)
//   (rocprim::exclusive_scan over the integer flags: integer addition is associative, its order cannot show)
//   k_knn_compact  the flagged rows at their place of the list -- ascending index --, and their number
//   k_knn_density  one lane per body, sequential: M = the masses of its first k - 1 neighbours added in list order from +0.0,
//                  r = sqrt(r2 of the k-th), rho = M / (4.1887902047863905 ((r r) r)); an incomplete row: +0.0 and +inf
// The pass over the cells of a grid, k_cells_knn, stands beside its siblings in kernels_cells.hip and keeps the same lists.
#include "kernels_knn.h"
#include "kernels_fof.h"   // pair_dist2
#include "knn_list.h"
#include "real.h"          // widen
#include "scratch_carve.h"

#include <rocprim/device/device_scan.hpp>

namespace nbody {

using knn::kPairBlock;

template <class F, int kSlots, bool kList>
__global__ __launch_bounds__(kPairBlock) void k_knn_pairs(const typename Real<F>::V4* __restrict__ pos, const int* __restrict__ count,
                                                          int n_upper, int groups, int K, int k, const int* __restrict__ list, int rows,
                                                          double* __restrict__ rec_r2, int* __restrict__ rec_j) {
    __shared__ double4 tx[kPairBlock];
    __shared__ knn::ListLds<kSlots> lists;
    const int tid = threadIdx.x;
    const int group = int(blockIdx.x) % groups, slice = int(blockIdx.x) / groups;
    const int n = live_count(count, n_upper);
    const int q = group * kPairBlock + tid;   // the row's place: rec is indexed by it
    int i = -1;
    if constexpr (kList) {
        if (q < rows) i = list[q];
    } else {
        if (q < n) i = q;
    }
    const bool live = i >= 0 && i < n;   // (a listed row is a live row; nothing is read outside pos whatever the list holds)
    const double4 pi = live ? widen(pos[i]) : make_double4(0.0, 0.0, 0.0, 0.0);
    const int lo = int((long long)n * slice / K), hi = int((long long)n * (slice + 1) / K);
    knn::ListState st;
    // pair_tiles.h's loop, written out: through for_each_partner the compiler folds the three tests below into one mask and
    // the pass over all rows measures 5% slower at k = 6
    for (int t0 = lo; t0 < hi; t0 += kPairBlock) {
        const int m = min(kPairBlock, hi - t0);
        __syncthreads();
        if (tid < m) tx[tid] = widen(pos[t0 + tid]);
        __syncthreads();
        for (int t = 0; t < m; ++t) {
            const double r2 = fof::pair_dist2(pi, tx[t]);   // wave-uniform addresses: LDS broadcasts
            if (r2 < st.last_r2 && t0 + t != i && live)     // (strict; a NaN or +inf never enters; the i == i pair is left out)
                knn::list_insert(lists, tid, k, st, r2, t0 + t);
        }
    }
    if (live) {
        const size_t stride = size_t(groups) * kPairBlock;
        for (int slot = 0; slot < k; ++slot) {
            const size_t at = (size_t(slice) * size_t(k) + size_t(slot)) * stride + size_t(q);
            rec_r2[at] = slot < st.held ? lists.r2[slot][tid] : inf64();
            rec_j[at] = slot < st.held ? lists.j[slot][tid] : -1;
        }
    }
}

template <int kSlots>
__global__ __launch_bounds__(kPairBlock) void k_knn_merge(const int* __restrict__ count, int n_upper, int K, int k, size_t stride,
                                                          const int* __restrict__ list, int rows, const double* __restrict__ rec_r2,
                                                          const int* __restrict__ rec_j, int* __restrict__ neighbor,
                                                          double* __restrict__ dist2) {
    __shared__ knn::ListLds<kSlots> lists;
    const int tid = threadIdx.x;
    const int q = blockIdx.x * kPairBlock + tid;
    const int n = live_count(count, n_upper);
    int i = -1;
    if (list) {
        if (q < rows) i = list[q];
    } else if (q < n) {
        i = q;
    }
    if (i < 0 || i >= n) return;   // (no barrier below: a lane's list is its own)
    knn::ListState st;
    for (int s = 0; s < K; ++s) {   // slices in ascending order hold ascending j
        for (int slot = 0; slot < k; ++slot) {
            const size_t at = (size_t(s) * size_t(k) + size_t(slot)) * stride + size_t(q);
            const int j = rec_j[at];
            if (j < 0) break;   // the padding: the slice's list ends here
            const double r2 = rec_r2[at];
            if (!(r2 < st.last_r2)) break;   // ascending within the slice: nothing after it enters either
            knn::list_insert(lists, tid, k, st, r2, j);
        }
    }
    for (int slot = 0; slot < k; ++slot) {
        neighbor[size_t(i) * size_t(k) + size_t(slot)] = slot < st.held ? lists.j[slot][tid] : -1;
        dist2[size_t(i) * size_t(k) + size_t(slot)] = slot < st.held ? lists.r2[slot][tid] : inf64();
    }
}

__global__ __launch_bounds__(kPairBlock) void k_knn_flag(const int* __restrict__ count, int n_upper, int k, const int* __restrict__ found,
                                                         int* __restrict__ flag) {
    const int i = blockIdx.x * kPairBlock + threadIdx.x;
    if (i >= n_upper) return;
    flag[i] = i < live_count(count, n_upper) && found[i] < k ? 1 : 0;
}

__global__ __launch_bounds__(kPairBlock) void k_knn_compact(int n_upper, const int* __restrict__ flag, const int* __restrict__ offset,
                                                            int* __restrict__ list, int* __restrict__ total) {
    const int i = blockIdx.x * kPairBlock + threadIdx.x;
    if (i >= n_upper) return;
    if (i == n_upper - 1) *total = offset[i] + flag[i];
    if (flag[i]) list[offset[i]] = i;   // (offset[i] < the flagged rows <= n_upper)
}

template <class F>
__global__ __launch_bounds__(kPairBlock) void k_knn_density(const typename Real<F>::V4* __restrict__ pos, const int* __restrict__ count,
                                                            int n_upper, int k, const int* __restrict__ neighbor,
                                                            const double* __restrict__ dist2, double* __restrict__ rho,
                                                            double* __restrict__ rk2) {
    const int i = blockIdx.x * kPairBlock + threadIdx.x;
    const int n = live_count(count, n_upper);
    if (i >= n) return;
    const int* mine = neighbor + size_t(i) * size_t(k);
    double d = 0.0, r2 = inf64();
    if (mine[k - 1] >= 0) {   // the list is complete
        double M = 0.0;
        for (int slot = 0; slot < k - 1; ++slot) {
            const int j = mine[slot];
            if (unsigned(j) < unsigned(n)) M += widen(pos[j]).w;   // (always: the lists hold live indices; no read outside pos whatever they hold)
        }
        r2 = dist2[size_t(i) * size_t(k) + size_t(k - 1)];
        const double r = __builtin_sqrt(r2);
        d = M / (4.1887902047863905 * ((r * r) * r));   // (r == 0: k coincident bodies; the IEEE result of the division)
    }
    if (rho) rho[i] = d;
    if (rk2) rk2[i] = r2;
}

namespace knn {

using pairs::blocks_for;

namespace {
void records(Carver& c, const PartnerPlan& p, int k, KnnScratch* w) {
    const size_t entries = size_t(p.K) * size_t(k) * size_t(p.groups) * kPairBlock;
    w->rec_r2 = c.take<double>(entries);
    w->rec_j = c.take<int>(entries);
}
KnnScratch layout(Carver& c, size_t n_upper, int k, bool cells) {
    KnnScratch w;
    w.dist2 = c.take<double>(n_upper * size_t(k));
    w.neighbor = c.take<int>(n_upper * size_t(k));
    if (cells) {
        w.found = c.take<int>(n_upper);
        w.flag = c.take<int>(n_upper);
        w.offset = c.take<int>(n_upper);
        w.list = c.take<int>(n_upper);
        w.total = c.take<int>(1);
        w.scan_bytes = pairs::scan_tmp_bytes(n_upper);
        w.scan_tmp = c.take<char>(w.scan_bytes);
    }
    return w;
}
}  // namespace

size_t scratch_bytes(size_t n_upper, int k, bool cells) { Carver c; layout(c, n_upper, k, cells); return c.offset(); }
KnnScratch scratch_layout(void* base, size_t n_upper, int k, bool cells) { Carver c(base); return layout(c, n_upper, k, cells); }

size_t record_bytes(const PartnerPlan& p, int k) { Carver c; KnnScratch w; records(c, p, k, &w); return c.offset(); }
void record_layout(void* base, const PartnerPlan& p, int k, KnnScratch* w) { Carver c(base); records(c, p, k, w); }

namespace {
template <class F, int kSlots>
void launch_pairs_slots(hipStream_t s, const ShardT<F>& sh, int n_upper, int k, const int* list, int rows, const PartnerPlan& p,
                        const KnnScratch& w) {
    const dim3 grid(unsigned(p.groups) * unsigned(p.K)), block(kPairBlock);
    if (list)
        hipLaunchKernelGGL((k_knn_pairs<F, kSlots, true>), grid, block, 0, s, sh.own_pos(), sh.own_count(), n_upper, p.groups, p.K, k, list,
                           rows, w.rec_r2, w.rec_j);
    else
        hipLaunchKernelGGL((k_knn_pairs<F, kSlots, false>), grid, block, 0, s, sh.own_pos(), sh.own_count(), n_upper, p.groups, p.K, k, list,
                           rows, w.rec_r2, w.rec_j);
    hipLaunchKernelGGL(k_knn_merge<kSlots>, dim3(unsigned(p.groups)), block, 0, s, sh.own_count(), n_upper, p.K, k,
                       size_t(p.groups) * kPairBlock, list, rows, w.rec_r2, w.rec_j, w.neighbor, w.dist2);
}
}  // namespace

template <class F>
void launch_pairs(hipStream_t s, const ShardT<F>& sh, int n_upper, int k, const int* list, int rows, const PartnerPlan& p, const KnnScratch& w) {
    if (n_upper <= 0 || rows <= 0 || p.groups <= 0 || k < 1 || k > kSlotsLarge) return;
    if (list_slots(k) == kSlotsSmall) launch_pairs_slots<F, kSlotsSmall>(s, sh, n_upper, k, list, rows, p, w);
    else launch_pairs_slots<F, kSlotsLarge>(s, sh, n_upper, k, list, rows, p, w);
}

int launch_unfinished(hipStream_t s, const int* live_count, int n_upper, int k, const KnnScratch& w) {
    if (n_upper <= 0) return 0;
    const int blocks = blocks_for(n_upper);
    hipLaunchKernelGGL(k_knn_flag, dim3(blocks), dim3(kPairBlock), 0, s, live_count, n_upper, k, w.found, w.flag);
    size_t tb = w.scan_bytes;
    if (rocprim::exclusive_scan(w.scan_tmp, tb, w.flag, w.offset, 0, size_t(n_upper), rocprim::plus<int>(), s) != hipSuccess) return -1;
    hipLaunchKernelGGL(k_knn_compact, dim3(blocks), dim3(kPairBlock), 0, s, n_upper, w.flag, w.offset, w.list, w.total);
    return 0;
}

template <class F>
void launch_density(hipStream_t s, const ShardT<F>& sh, int n_upper, int k, const KnnScratch& w, double* rho, double* rk2) {
    if (n_upper <= 0 || k < 1) return;
    hipLaunchKernelGGL(k_knn_density<F>, dim3(blocks_for(n_upper)), dim3(kPairBlock), 0, s, sh.own_pos(), sh.own_count(), n_upper, k,
                       w.neighbor, w.dist2, rho, rk2);
}

template void launch_pairs<float>(hipStream_t, const ShardT<float>&, int, int, const int*, int, const PartnerPlan&, const KnnScratch&);
template void launch_pairs<double>(hipStream_t, const ShardT<double>&, int, int, const int*, int, const PartnerPlan&, const KnnScratch&);
template void launch_density<float>(hipStream_t, const ShardT<float>&, int, int, const KnnScratch&, double*, double*);
template void launch_density<double>(hipStream_t, const ShardT<double>&, int, int, const KnnScratch&, double*, double*);

}}  // namespace nbody::knn
