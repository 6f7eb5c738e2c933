// kernels_fof.hip -- friends-of-friends groups of a handle's bodies on the device (gfx950): nbody_fof_labels and
// nbody_fof_groups (include/nbody_hip.h, "friends-of-friends groups").  Compiled with -ffp-contract=off (every product, sum
// and difference rounded on its own).  No floating-point atomics: the same input gives the same bits.  Every kernel reads the
// handle's state and writes the call's scratch only.
//
// THE INVARIANT of parent[] (fof_union.h has the full argument): parent[x] <= x, a word only ever decreases, and it always
// names a body of x's own component.  So a stale read -- the per-XCD L2s are not coherent with each other and a CU's L1 is
// never refreshed by other CUs -- costs steps, never correctness: every chain strictly descends and ends, and when k_fof_link
// has finished the one root of a component is its lowest index.  Inside k_fof_link every write to parent[] is an atomicCAS or
// an atomicMin that lowers the word, every read is a relaxed agent-scope atomic load (served by L2, not by the CU's L1), and
// no lane ever waits for another lane, wave or workgroup: no lock, no spin on a flag, and the only retry follows a lost CAS,
// which means someone else lowered the word.
//
//   k_fof_init     parent[i] = i for live rows, -1 beyond the live count; size[i] = 0
//   k_fof_link     the all-pairs pass on k_partner<F, true>'s frame: one body per lane (its position in registers as doubles),
//                  the partners of a slice staged through LDS in tiles of 256, the grid (groups of 256 bodies) x K slices.
//                  r2_ij == r2_ji bit for bit, so only j > i is looked at, and a block whose whole partner range lies at or
//                  below its own bodies returns at once.  Where r2 < B2 the lane unites i and j (fof_union.h)
//   k_fof_flatten  after the kernel boundary: label[i] = the root of i, and size[root] counted with an integer atomicAdd (an
//                  integer: the order cannot show)
//   k_fof_flag     flag = 1 on roots with size >= min_members, listed = their size
//   (rocprim::exclusive_scan: flags -> group slots, listed sizes -> offsets into the member list)
//   k_fof_slots    slot_root[slot] = the root; every row's sort key = its group's slot, or INT_MAX; the two totals
//   (rocprim::radix_sort_pairs, stable, on (key, row): the member list, group after group in ascending slot = ascending first,
//   each group in ascending row)
//   k_fof_sums     one wave per listed group: the seven sums in the order the header fixes, and the NbodyGroup record
#include "kernels_fof.h"
#include "fof_union.h"
#include "pair_tiles.h"
#include "real.h"      // widen
#include "scratch_carve.h"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <climits>

namespace nbody {

using pairs::kPairBlock;
using fof::DevParent;     // kernels_fof.h: shared with k_cells_link
using fof::pair_dist2;

__global__ __launch_bounds__(kPairBlock) void k_fof_init(const int* __restrict__ count, int n_upper, int* __restrict__ parent,
                                                         int* __restrict__ size) {
    const int i = blockIdx.x * kPairBlock + threadIdx.x;
    if (i >= n_upper) return;
    parent[i] = i < live_count(count, n_upper) ? i : -1;
    size[i] = 0;
}

template <class F>
__global__ __launch_bounds__(kPairBlock) void k_fof_link(const typename Real<F>::V4* __restrict__ pos, const int* __restrict__ count,
                                                         int n_upper, int groups, int K, double B2, int* parent) {
    __shared__ double4 tx[kPairBlock];
    const int n = live_count(count, n_upper);
    pairs::PairFrame f(groups, K, n);
    if (!f.triangle()) return;   // (block-uniform: no partner j > i for any of its bodies)
    const int i = f.first + int(threadIdx.x);
    const bool live = i < n;
    const int mine = live ? i : INT_MAX;   // (no j is above it: a lane without a body links nothing)
    const double4 pi = live ? widen(pos[i]) : make_double4(0.0, 0.0, 0.0, 0.0);
    const DevParent forest{parent};
    pairs::for_each_partner(
        f, [&](int slot, int j) { tx[slot] = widen(pos[j]); },   // (j < hi <= n <= n_upper)
        [&](int j, int t) {
            const double r2 = pair_dist2(pi, tx[t]);
            if (r2 < B2 && j > mine) fof::fof_link(forest, i, j);   // (strict; a NaN never links)
        });
}

__global__ __launch_bounds__(kPairBlock) void k_fof_flatten(const int* __restrict__ count, int n_upper, const int* __restrict__ parent,
                                                            int* __restrict__ label, int* __restrict__ size) {
    const int i = blockIdx.x * kPairBlock + threadIdx.x;
    if (i >= n_upper) return;
    int r = -1;
    if (i < live_count(count, n_upper)) {
        r = i;
        for (int p = parent[r]; p != r; p = parent[r]) r = p;   // (0 <= parent[r] < r: the chain descends to the root)
        atomicAdd(&size[r], 1);
    }
    label[i] = r;
}

__global__ __launch_bounds__(kPairBlock) void k_fof_flag(int n_upper, int min_members, const int* __restrict__ label,
                                                         const int* __restrict__ size, int* __restrict__ flag, int* __restrict__ listed) {
    const int i = blockIdx.x * kPairBlock + threadIdx.x;
    if (i >= n_upper) return;
    const int f = label[i] == i && size[i] >= min_members;   // (rows past the live count carry label -1)
    flag[i] = f;
    listed[i] = f ? size[i] : 0;
}

__global__ __launch_bounds__(kPairBlock) void k_fof_slots(int n_upper, const int* __restrict__ label, const int* __restrict__ flag,
                                                          const int* __restrict__ listed, const int* __restrict__ slot,
                                                          const int* __restrict__ offset, int* __restrict__ slot_root,
                                                          unsigned* __restrict__ keys, int* __restrict__ rows, int* __restrict__ total) {
    const int i = blockIdx.x * kPairBlock + threadIdx.x;
    if (i >= n_upper) return;
    if (i == n_upper - 1) {
        total[0] = slot[i] + flag[i];
        total[1] = offset[i] + listed[i];
    }
    if (flag[i]) slot_root[slot[i]] = i;   // (slot < the listed groups <= n_upper)
    const int r = label[i];
    keys[i] = r >= 0 && flag[r] ? unsigned(slot[r]) : unsigned(INT_MAX);
    rows[i] = i;
}

// One wave per listed group, members k = 0 .. count-1 in ascending index: the seven sums in the header's order (seven_sums of
// kernels_fof.h), and the record.
template <class F>
__global__ __launch_bounds__(kPairBlock) void k_fof_sums(const typename Real<F>::V4* __restrict__ pos,
                                                         const typename Real<F>::V4* __restrict__ vel, int n_groups,
                                                         const int* __restrict__ size, const int* __restrict__ offset,
                                                         const int* __restrict__ slot_root, const int* __restrict__ members,
                                                         NbodyGroup* __restrict__ out) {
    const int lane = threadIdx.x % 64;
    const int g = blockIdx.x * (kPairBlock / 64) + threadIdx.x / 64;
    if (g >= n_groups) return;   // (wave-uniform)
    const int root = slot_root[g];
    const int cnt = size[root], off = offset[root];
    double s[7];
    fof::seven_sums<F>(pos, vel, members + off, cnt, nullptr, lane, s);
    if (lane == 0) {
        NbodyGroup r;
        r.first = root;
        r.count = cnt;
        r.offset = off;
        r.reserved = 0;
        r.mass = s[0];
        for (int c = 0; c < 3; ++c) {
            r.mx[c] = s[1 + c];
            r.mv[c] = s[4 + c];
        }
        out[g] = r;
    }
}

namespace fof {

namespace {
size_t sort_tmp_bytes(size_t n_upper) {
    size_t b = 0;
    unsigned* k = nullptr;
    int* v = nullptr;
    (void)rocprim::radix_sort_pairs(nullptr, b, k, k, v, v, n_upper, 0, 31, 0);
    return b;
}
FofScratch layout(Carver& c, size_t n_upper) {
    FofScratch w;
    for (int** p : {&w.parent, &w.label, &w.size, &w.flag, &w.listed, &w.slot, &w.offset, &w.slot_root}) *p = c.take<int>(n_upper);
    w.keys = c.take<unsigned>(2 * n_upper);
    w.rows = c.take<int>(2 * n_upper);
    w.total = c.take<int>(2);
    w.scan_bytes = pairs::scan_tmp_bytes(n_upper);
    w.scan_tmp = c.take<char>(w.scan_bytes);
    w.sort_bytes = sort_tmp_bytes(n_upper);
    w.sort_tmp = c.take<char>(w.sort_bytes);
    return w;
}
}  // namespace

size_t scratch_bytes(size_t n_upper) { Carver c; layout(c, n_upper); return c.offset(); }
FofScratch scratch_layout(void* base, size_t n_upper) { Carver c(base); return layout(c, n_upper); }

template <class F>
void launch_components(hipStream_t s, const ShardT<F>& sh, int n_upper, const pairs::PartnerPlan& p, double B2, const FofScratch& w) {
    if (n_upper <= 0 || p.groups <= 0) return;
    launch_forest_init(s, sh.own_count(), n_upper, w);
    hipLaunchKernelGGL(k_fof_link<F>, dim3(unsigned(p.groups) * unsigned(p.K)), dim3(kPairBlock), 0, s, sh.own_pos(), sh.own_count(),
                       n_upper, p.groups, p.K, B2, w.parent);
    launch_flatten(s, sh.own_count(), n_upper, w);
}

void launch_forest_init(hipStream_t s, const int* count, int n_upper, const FofScratch& w) {
    if (n_upper <= 0) return;
    hipLaunchKernelGGL(k_fof_init, dim3(pairs::blocks_for(n_upper)), dim3(kPairBlock), 0, s, count, n_upper, w.parent, w.size);
}

void launch_flatten(hipStream_t s, const int* count, int n_upper, const FofScratch& w) {
    if (n_upper <= 0) return;
    hipLaunchKernelGGL(k_fof_flatten, dim3(pairs::blocks_for(n_upper)), dim3(kPairBlock), 0, s, count, n_upper, w.parent, w.label, w.size);
}

int launch_catalogue(hipStream_t s, int n_upper, int min_members, bool sort, const FofScratch& w) {
    if (n_upper <= 0) return 0;
    const int blocks = pairs::blocks_for(n_upper);
    hipLaunchKernelGGL(k_fof_flag, dim3(blocks), dim3(kPairBlock), 0, s, n_upper, min_members, w.label, w.size, w.flag, w.listed);
    size_t tb = w.scan_bytes;
    if (rocprim::exclusive_scan(w.scan_tmp, tb, w.flag, w.slot, 0, size_t(n_upper), rocprim::plus<int>(), s) != hipSuccess) return -1;
    tb = w.scan_bytes;
    if (rocprim::exclusive_scan(w.scan_tmp, tb, w.listed, w.offset, 0, size_t(n_upper), rocprim::plus<int>(), s) != hipSuccess) return -1;
    hipLaunchKernelGGL(k_fof_slots, dim3(blocks), dim3(kPairBlock), 0, s, n_upper, w.label, w.flag, w.listed, w.slot, w.offset,
                       w.slot_root, w.keys, w.rows, w.total);
    if (!sort) return 0;
    tb = w.sort_bytes;
    if (rocprim::radix_sort_pairs(w.sort_tmp, tb, w.keys, w.keys + n_upper, w.rows, w.rows + n_upper, size_t(n_upper), 0, 31, s) != hipSuccess)
        return -1;
    return 0;
}

template <class F>
void launch_sums(hipStream_t s, const ShardT<F>& sh, int n_upper, int n_groups, const FofScratch& w, NbodyGroup* out) {
    if (n_groups <= 0) return;
    const int waves_per_block = kPairBlock / 64;
    hipLaunchKernelGGL(k_fof_sums<F>, dim3((n_groups + waves_per_block - 1) / waves_per_block), dim3(kPairBlock), 0, s, sh.own_pos(), sh.vel,
                       n_groups, w.size, w.offset, w.slot_root, w.members(size_t(n_upper)), out);
}

template void launch_components<float>(hipStream_t, const ShardT<float>&, int, const pairs::PartnerPlan&, double, const FofScratch&);
template void launch_components<double>(hipStream_t, const ShardT<double>&, int, const pairs::PartnerPlan&, double, const FofScratch&);
template void launch_sums<float>(hipStream_t, const ShardT<float>&, int, int, const FofScratch&, NbodyGroup*);
template void launch_sums<double>(hipStream_t, const ShardT<double>&, int, int, const FofScratch&, NbodyGroup*);

}}  // namespace nbody::fof
