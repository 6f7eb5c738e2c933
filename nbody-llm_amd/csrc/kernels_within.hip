// kernels_within.hip -- the fixed-radius neighbour lists of nbody_neighbors_within, and nbody_density and
// nbody_density_center on top of them (include/nbody_hip.h, "neighbours within a radius"), on the device (gfx950), f64 on
// either dtype.  Compiled with -ffp-contract=off (every product, sum and difference rounded on its own; sqrt and divide are
// IEEE).  No floating-point atomics: the same state gives the same bits.  Every kernel reads the handle's state and writes the
// call's scratch only.
//
//   k_within_pairs    the all-pairs pass on k_partner's frame: one body per lane, the partners of a slice staged through LDS in
//                     tiles of 256, j ascending; the grid is (groups of 256 bodies) x K slices.  kFill == false counts the
//                     j != i with r2 < R2 of (body, slice) into count[i K + slice] and adds them up in 64 bits (shuffles, one
//                     integer atomicAdd per wave); kFill == true evaluates the same r2 again and writes the j of the slice at
//                     place[i K + slice] on -- ascending within a slice, and the slices of a body stand in ascending order, so
//                     a body's list is ascending whatever K is
//   (rocprim::exclusive_scan over the integer counts, body-major: integer addition is associative, its order cannot show)
//   k_within_offsets  offset[i] = place[i K] for K > 1
//   (rocprim::segmented_radix_sort_keys for the lists that kernels_cells.hip's k_cells_within filled cell by cell: integer
//   keys, distinct within a segment)
//   k_within_density  one lane per body walks its list sequentially: the neighbours in ascending index and the body's own term
//                     at u = 0 where its index falls among them, every term added to one running sum that starts at +0.0
//   k_within_center   one body per lane, four LDS sums of 256 doubles, k_diag_moments' pairwise tree per block
#include "kernels_within.h"
#include "kernels_fof.h"   // pair_dist2
#include "pair_tiles.h"
#include "real.h"          // widen
#include "scratch_carve.h"

#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_segmented_radix_sort.hpp>

#include <algorithm>

namespace nbody {

using within::kCenterSums;
using within::kPairBlock;

template <class F, bool kFill>
__global__ __launch_bounds__(kPairBlock) void k_within_pairs(const typename Real<F>::V4* __restrict__ pos, const int* __restrict__ count,
                                                             int n_upper, int groups, int K, double R2, int* __restrict__ cnt,
                                                             const int* __restrict__ place, int* __restrict__ neighbor,
                                                             unsigned cap, unsigned long long* total) {
    __shared__ double4 tx[kPairBlock];
    const int n = live_count(count, n_upper);
    const pairs::PairFrame f(groups, K, n);
    const int i = f.first + int(threadIdx.x);
    const bool live = i < n;
    const double4 pi = live ? widen(pos[i]) : make_double4(0.0, 0.0, 0.0, 0.0);
    unsigned at = kFill && live ? unsigned(place[size_t(i) * K + f.slice]) : 0u;
    int found = 0;
    pairs::for_each_partner(
        f, [&](int slot, int j) { tx[slot] = widen(pos[j]); },
        [&](int j, int t) {
            const double r2 = fof::pair_dist2(pi, tx[t]);
            if (r2 < R2 && j != i && live) {           // (strict; a NaN is never within R)
                if constexpr (kFill) {
                    if (at < cap) neighbor[at] = j;    // (at < cap always: the count pass saw the same state)
                    ++at;
                } else {
                    ++found;
                }
            }
        });
    if constexpr (!kFill) {
        if (i < n_upper) cnt[size_t(i) * K + f.slice] = found;   // (rows past the live count: 0)
        wave_add((unsigned long long)found, total);             // (every lane of the wave is here)
    }
}

__global__ __launch_bounds__(kPairBlock) void k_within_offsets(int n_upper, int K, const int* __restrict__ place, int* __restrict__ offset) {
    const int i = blockIdx.x * kPairBlock + threadIdx.x;
    if (i <= n_upper) offset[i] = place[size_t(i) * K];
}

namespace {
// the M4 spline of Monaghan & Lattanzio at u = r / hs in [0, 2], without its normalisation
__device__ __forceinline__ double spline_w(double u) {
    if (u < 1.0) return (1.0 - 1.5 * (u * u)) + 0.75 * ((u * u) * u);
    const double t = 2.0 - u;   // (>= 0: sqrt(r2) <= sqrt(fl(radius radius)) == radius)
    return 0.25 * ((t * t) * t);
}
}  // namespace

template <class F, bool kSpline>
__global__ __launch_bounds__(kPairBlock) void k_within_density(const typename Real<F>::V4* __restrict__ pos, const int* __restrict__ count,
                                                               int n_upper, double hs, double norm, const int* __restrict__ offset,
                                                               const int* __restrict__ neighbor, double* __restrict__ rho,
                                                               int* __restrict__ terms) {
    const int i = blockIdx.x * kPairBlock + threadIdx.x;
    const int n = live_count(count, n_upper);
    if (i >= n) return;
    const double4 pi = widen(pos[i]);
    const double own = kSpline ? pi.w * spline_w(0.0) : pi.w;   // the body's own term: u = 0, no r2
    const int a = offset[i], b = offset[i + 1];
    double s = 0.0;
    bool own_added = false;
    for (int k = a; k < b; ++k) {   // ascending j
        const int j = neighbor[k];
        if (unsigned(j) >= unsigned(n)) continue;   // (never: the lists hold live indices; no read outside pos whatever they hold)
        if (!own_added && j > i) { s += own; own_added = true; }
        const double4 pj = widen(pos[j]);
        if constexpr (kSpline) s += pj.w * spline_w(__builtin_sqrt(fof::pair_dist2(pi, pj)) / hs);
        else s += pj.w;
    }
    if (!own_added) s += own;
    if (rho) rho[i] = s / norm;
    if (terms) terms[i] = (b - a) + 1;
}

template <class F>
__global__ __launch_bounds__(kPairBlock) void k_within_center(const typename Real<F>::V4* __restrict__ pos, const int* __restrict__ count,
                                                              int n_upper, const double* __restrict__ rho, double* __restrict__ part) {
    __shared__ double sum[kCenterSums][kPairBlock];
    const int t = threadIdx.x;
    const int i = blockIdx.x * kPairBlock + t;
    double term[kCenterSums] = {0.0, 0.0, 0.0, 0.0};
    if (i < live_count(count, n_upper)) {
        const double4 p = widen(pos[i]);
        const double r = rho[i];
        term[0] = r;
        term[1] = r * p.x;
        term[2] = r * p.y;
        term[3] = r * p.z;
    }
#pragma unroll
    for (int q = 0; q < kCenterSums; ++q) sum[q][t] = term[q];
    __syncthreads();
    for (int half = kPairBlock / 2; half > 0; half >>= 1) {   // sum[t] += sum[t + half]: the same pairs whatever the schedule
        if (t < half) {
#pragma unroll
            for (int q = 0; q < kCenterSums; ++q) sum[q][t] = sum[q][t] + sum[q][t + half];
        }
        __syncthreads();
    }
    if (t < kCenterSums) part[size_t(blockIdx.x) * kCenterSums + t] = sum[t][0];
}

namespace within {

using pairs::blocks_for;

namespace {
// the bits that hold every index below n_upper
unsigned key_bits(size_t n_upper) {
    unsigned bits = 1;
    while (bits < 31 && (size_t(1) << bits) < n_upper) ++bits;
    return bits;
}
size_t sort_tmp_bytes(size_t n_upper, size_t total) {
    size_t b = 0;
    int* v = nullptr;
    (void)rocprim::segmented_radix_sort_keys(nullptr, b, v, v, unsigned(total), unsigned(n_upper), v, v, 0, key_bits(n_upper), 0);
    return b;
}
CountScratch count_layout(Carver& at, size_t n_upper, int K) {
    CountScratch c;
    c.words = n_upper * size_t(K) + 1;
    c.total = at.take<unsigned long long>(1);
    c.count = at.take<int>(c.words);
    c.place = at.take<int>(c.words);
    c.offset = K > 1 ? at.take<int>(n_upper + 1) : c.place;
    c.scan_bytes = pairs::scan_tmp_bytes(c.words);
    c.scan_tmp = at.take<char>(c.scan_bytes);
    return c;
}
ListScratch list_layout(Carver& at, size_t n_upper, size_t total, bool sorted) {
    ListScratch l;
    l.neighbor = at.take<int>(total);
    if (sorted) {
        l.raw = at.take<int>(total);
        l.sort_bytes = sort_tmp_bytes(n_upper, total);
        l.sort_tmp = at.take<char>(l.sort_bytes);
    }
    return l;
}
}  // namespace

size_t count_scratch_bytes(size_t n_upper, int K) { Carver at; count_layout(at, n_upper, K); return at.offset(); }
CountScratch count_scratch_layout(void* base, size_t n_upper, int K) { Carver at(base); return count_layout(at, n_upper, K); }

size_t list_scratch_bytes(size_t n_upper, size_t total, bool sorted) { Carver at; list_layout(at, n_upper, total, sorted); return at.offset(); }
ListScratch list_scratch_layout(void* base, size_t n_upper, size_t total, bool sorted) {
    Carver at(base);
    return list_layout(at, n_upper, total, sorted);
}

void launch_clear(hipStream_t s, const CountScratch& c) {
    (void)hipMemsetAsync(c.total, 0, sizeof(unsigned long long), s);
    (void)hipMemsetAsync(c.count, 0, c.words * sizeof(int), s);
}

template <class F>
void launch_count_pairs(hipStream_t s, const ShardT<F>& sh, int n_upper, const PartnerPlan& p, double R2, const CountScratch& c) {
    if (n_upper <= 0 || p.groups <= 0) return;
    hipLaunchKernelGGL((k_within_pairs<F, false>), dim3(unsigned(p.groups) * unsigned(p.K)), dim3(kPairBlock), 0, s, sh.own_pos(),
                       sh.own_count(), n_upper, p.groups, p.K, R2, c.count, static_cast<const int*>(nullptr), static_cast<int*>(nullptr), 0u,
                       c.total);
}

int launch_places(hipStream_t s, int n_upper, int K, const CountScratch& c) {
    size_t tb = c.scan_bytes;
    if (rocprim::exclusive_scan(c.scan_tmp, tb, c.count, c.place, 0, c.words, rocprim::plus<int>(), s) != hipSuccess) return -1;
    if (K > 1)
        hipLaunchKernelGGL(k_within_offsets, dim3(blocks_for(n_upper + 1)), dim3(kPairBlock), 0, s, n_upper, K, c.place, c.offset);
    return 0;
}

template <class F>
void launch_fill_pairs(hipStream_t s, const ShardT<F>& sh, int n_upper, const PartnerPlan& p, double R2, const CountScratch& c,
                       const ListScratch& l, size_t total) {
    if (n_upper <= 0 || p.groups <= 0 || !total) return;
    hipLaunchKernelGGL((k_within_pairs<F, true>), dim3(unsigned(p.groups) * unsigned(p.K)), dim3(kPairBlock), 0, s, sh.own_pos(),
                       sh.own_count(), n_upper, p.groups, p.K, R2, static_cast<int*>(nullptr), c.place, l.neighbor, unsigned(total),
                       static_cast<unsigned long long*>(nullptr));
}

int launch_sort_lists(hipStream_t s, int n_upper, const CountScratch& c, const ListScratch& l, size_t total) {
    if (n_upper <= 0 || !total) return 0;
    size_t tb = l.sort_bytes;
    return rocprim::segmented_radix_sort_keys(l.sort_tmp, tb, l.raw, l.neighbor, unsigned(total), unsigned(n_upper), c.offset, c.offset + 1,
                                              0, key_bits(size_t(n_upper)), s) == hipSuccess ? 0 : -1;
}

template <class F>
void launch_density(hipStream_t s, const ShardT<F>& sh, int n_upper, bool spline, double hs, double norm, const int* offset,
                    const int* neighbor, double* rho, int* count) {
    if (n_upper <= 0) return;
    if (spline)
        hipLaunchKernelGGL((k_within_density<F, true>), dim3(blocks_for(n_upper)), dim3(kPairBlock), 0, s, sh.own_pos(), sh.own_count(), n_upper,
                           hs, norm, offset, neighbor, rho, count);
    else
        hipLaunchKernelGGL((k_within_density<F, false>), dim3(blocks_for(n_upper)), dim3(kPairBlock), 0, s, sh.own_pos(), sh.own_count(), n_upper,
                           hs, norm, offset, neighbor, rho, count);
}

template <class F>
void launch_center(hipStream_t s, const ShardT<F>& sh, int n_upper, const double* rho, double* part) {
    if (n_upper <= 0) return;
    hipLaunchKernelGGL(k_within_center<F>, dim3(blocks_for(n_upper)), dim3(kPairBlock), 0, s, sh.own_pos(), sh.own_count(), n_upper, rho, part);
}

template void launch_count_pairs<float>(hipStream_t, const ShardT<float>&, int, const PartnerPlan&, double, const CountScratch&);
template void launch_count_pairs<double>(hipStream_t, const ShardT<double>&, int, const PartnerPlan&, double, const CountScratch&);
template void launch_fill_pairs<float>(hipStream_t, const ShardT<float>&, int, const PartnerPlan&, double, const CountScratch&, const ListScratch&, size_t);
template void launch_fill_pairs<double>(hipStream_t, const ShardT<double>&, int, const PartnerPlan&, double, const CountScratch&, const ListScratch&, size_t);
template void launch_density<float>(hipStream_t, const ShardT<float>&, int, bool, double, double, const int*, const int*, double*, int*);
template void launch_density<double>(hipStream_t, const ShardT<double>&, int, bool, double, double, const int*, const int*, double*, int*);
template void launch_center<float>(hipStream_t, const ShardT<float>&, int, const double*, double*);
template void launch_center<double>(hipStream_t, const ShardT<double>&, int, const double*, double*);

}}  // namespace nbody::within
