// kernels_unbind.hip -- iterative unbinding of friends-of-friends groups on the device (gfx950): nbody_fof_bound_groups
// (include/nbody_hip.h, "self-bound subsets of friends-of-friends groups").  Compiled with -ffp-contract=off (every product, sum
// and difference rounded on its own; sqrt and divide are IEEE).  No floating-point atomics: the same input gives the same bits.
// Every kernel reads the handle's state and the FoF catalogue (kernels_fof.hip) and writes the call's scratch only.
//
// The FoF member list holds the listed groups one after another, each in ascending index; a member's POSITION p in that list
// and its position k = p - offset in its own group never change while flags are cleared, so every order below is fixed by the
// catalogue alone.
//
//   k_unbind_init     alive[p] = 1; every group running with all its members
//   k_unbind_sums     one wave per running group: the seven sums of its alive members (seven_sums of kernels_fof.h)
//   k_unbind_energy   THE HOT KERNEL.  One member per lane, block b owns positions 256 b .. 256 b + 255 of the member list, so a
//                     group of n_g members is spread over n_g / 256 blocks (a group far larger than the rest is not one
//                     block's work), and the grid does not depend on any knob.  The partners of a member are the positions
//                     k = 0 .. fof_count-1 of its own group in tiles of 256 (k div 256): p = +0.0 per tile, s += p per tile.
//                     Where all rows of a block lie in one group (every block inside a large group) the tile is staged through
//                     LDS once for the 256 rows -- positions widened, the mass in .w, the flags beside them -- and read back
//                     at wave-uniform addresses (broadcasts).  A block that straddles groups (small groups, and the two ends
//                     of a large one) lets each lane walk its own group from global memory: the same terms in the same order.
//                     A dead partner is skipped by a wave-uniform branch in the LDS path.  Rows that are dead or whose group has
//                     stopped do nothing; a block whose one group has stopped returns at once.
//   k_unbind_verdict  one wave per running group: counts the unbound (integers), stops the group or clears their flags at once
//   k_unbind_keep     mark[p] = reported; keep / kept per group
//   (rocprim::exclusive_scan x 3: the reported groups' slots and offsets, the reported members' places)
//   k_unbind_compact  the reported members and their energies, in the order of the FoF member list
//   k_unbind_records  one wave per reported group: kinetic and potential in seven_sums' shape, and the NbodyBoundGroup record
#include "kernels_unbind.h"
#include "real.h"   // widen
#include "scratch_carve.h"

#include <rocprim/device/device_scan.hpp>

#include <algorithm>

namespace nbody {

using fof::UnbindGroup;
using pairs::kPairBlock;

namespace {

// m_k / sqrt(r2), r2 = ((dx dx + dy dy) + dz dz) + soft2: nbody_partners' softened r2
__device__ __forceinline__ double partner_term(const double4 pi, const double4 pk, double soft2) {
    const double dx = pk.x - pi.x, dy = pk.y - pi.y, dz = pk.z - pi.z;
    const double r2 = ((dx * dx + dy * dy) + dz * dz) + soft2;
    return pk.w / __builtin_sqrt(r2);
}

__device__ __forceinline__ int wave_sum(int v) {
    for (int half = 32; half >= 1; half >>= 1) v += __shfl_xor(v, half, 64);
    return v;
}

}  // namespace

__global__ __launch_bounds__(kPairBlock) void k_unbind_init(int n_members, int n_groups, const int* __restrict__ size,
                                                            const int* __restrict__ slot_root, UnbindGroup* __restrict__ grp,
                                                            int* __restrict__ alive) {
    const int i = blockIdx.x * kPairBlock + threadIdx.x;
    if (i < n_members) alive[i] = 1;
    if (i < n_groups) {
        UnbindGroup g;
        g.running = 1;
        g.iterations = 0;
        g.converged = 0;
        g.alive = size[slot_root[i]];
        for (int c = 0; c < 7; ++c) g.sum[c] = 0.0;
        grp[i] = g;
    }
}

template <class F>
__global__ __launch_bounds__(kPairBlock) void k_unbind_sums(const typename Real<F>::V4* __restrict__ pos,
                                                            const typename Real<F>::V4* __restrict__ vel, int n_groups,
                                                            const int* __restrict__ size, const int* __restrict__ offset,
                                                            const int* __restrict__ slot_root, const int* __restrict__ members,
                                                            const int* __restrict__ alive, UnbindGroup* __restrict__ grp) {
    const int lane = threadIdx.x % 64;
    const int g = blockIdx.x * (kPairBlock / 64) + threadIdx.x / 64;
    if (g >= n_groups || !grp[g].running) return;   // (wave-uniform)
    const int root = slot_root[g];
    const int off = offset[root];
    double s[7];
    fof::seven_sums<F>(pos, vel, members + off, size[root], alive + off, lane, s);
    if (lane == 0)
        for (int c = 0; c < 7; ++c) grp[g].sum[c] = s[c];
}

template <class F>
__global__ __launch_bounds__(kPairBlock) void k_unbind_energy(const typename Real<F>::V4* __restrict__ pos,
                                                              const typename Real<F>::V4* __restrict__ vel, int n_members,
                                                              const int* __restrict__ size, const int* __restrict__ offset,
                                                              const int* __restrict__ slot_root, const int* __restrict__ members,
                                                              const unsigned* __restrict__ group_of, const UnbindGroup* __restrict__ grp,
                                                              const int* __restrict__ alive, double g, double soft2,
                                                              double* __restrict__ energy, double* __restrict__ kinetic,
                                                              double* __restrict__ potential, int* __restrict__ mark) {
    __shared__ double4 tx[kPairBlock];
    __shared__ int ta[kPairBlock];
    const int tid = threadIdx.x;
    const int p0 = blockIdx.x * kPairBlock;   // (p0 < n_members: the grid is blocks_for(n_members))
    const int p = p0 + tid;
    const int g_first = int(group_of[p0]), g_last = int(group_of[min(p0 + kPairBlock, n_members) - 1]);
    const bool one_group = g_first == g_last;   // (block-uniform; the list is sorted by group)
    if (one_group && !grp[g_first].running) return;
    const int gi = p < n_members ? int(group_of[p]) : g_first;
    const int root = slot_root[gi];
    const int off = offset[root], cnt = size[root];   // (a lane past the list takes the first row's group: it only helps to stage)
    const int k_i = p - off;
    const bool act = p < n_members && grp[gi].running && alive[p];
    const double4 xi = act ? widen(pos[members[p]]) : make_double4(0.0, 0.0, 0.0, 0.0);
    double s = 0.0;
    if (one_group) {
        for (int t0 = 0; t0 < cnt; t0 += kPairBlock) {
            const int n_t = min(kPairBlock, cnt - t0);
            __syncthreads();
            if (tid < n_t) {   // (off + t0 + tid < off + cnt <= n_members)
                tx[tid] = widen(pos[members[off + t0 + tid]]);
                ta[tid] = alive[off + t0 + tid];
            }
            __syncthreads();
            if (act) {
                double part = 0.0;
                for (int t = 0; t < n_t; ++t)   // wave-uniform addresses: LDS broadcasts
                    if (ta[t] && t0 + t != k_i) part += partner_term(xi, tx[t], soft2);
                s += part;
            }
        }
    } else if (act) {
        for (int t0 = 0; t0 < cnt; t0 += kPairBlock) {
            const int n_t = min(kPairBlock, cnt - t0);
            double part = 0.0;
            for (int t = 0; t < n_t; ++t)
                if (alive[off + t0 + t] && t0 + t != k_i) part += partner_term(xi, widen(pos[members[off + t0 + t]]), soft2);
            s += part;
        }
    }
    if (!act) return;
    const double4 vi = widen(vel[members[p]]);
    const double* sum = grp[gi].sum;
    const double ux = vi.x - sum[4] / sum[0], uy = vi.y - sum[5] / sum[0], uz = vi.z - sum[6] / sum[0];
    const double u2 = (ux * ux + uy * uy) + uz * uz;
    const double phi = -(g * s);
    const double e = 0.5 * u2 + phi;
    const double hm = 0.5 * xi.w;
    energy[p] = e;
    kinetic[p] = hm * u2;
    potential[p] = hm * phi;
    mark[p] = !(e < 0.0);   // (a NaN energy is unbound, -inf is bound)
}

__global__ __launch_bounds__(kPairBlock) void k_unbind_verdict(int n_groups, int min_members, int pass, int last,
                                                               const int* __restrict__ size, const int* __restrict__ offset,
                                                               const int* __restrict__ slot_root, UnbindGroup* __restrict__ grp,
                                                               int* __restrict__ alive, const int* __restrict__ mark,
                                                               int* __restrict__ counters) {
    const int lane = threadIdx.x % 64;
    const int g = blockIdx.x * (kPairBlock / 64) + threadIdx.x / 64;
    if (g >= n_groups || !grp[g].running) return;   // (wave-uniform)
    const int root = slot_root[g];
    const int off = offset[root], cnt = size[root];
    int unbound = 0;
    for (int k = lane; k < cnt; k += 64) unbound += alive[off + k] && mark[off + k];
    unbound = wave_sum(unbound);
    const bool strip = unbound && !last;
    if (strip)   // every unbound member of the pass at once
        for (int k = lane; k < cnt; k += 64)
            if (alive[off + k] && mark[off + k]) alive[off + k] = 0;
    if (lane) return;
    const int left = grp[g].alive - (strip ? unbound : 0);
    const bool on = strip && left >= min_members;
    grp[g].iterations = pass + 1;
    grp[g].converged = !unbound;
    grp[g].alive = left;
    grp[g].running = on;
    if (on) atomicAdd(counters, 1);   // (an integer: the order cannot show)
}

__global__ __launch_bounds__(kPairBlock) void k_unbind_keep(int n_members, int n_groups, int min_members,
                                                            const unsigned* __restrict__ group_of, const UnbindGroup* __restrict__ grp,
                                                            const int* __restrict__ alive, int* __restrict__ mark, int* __restrict__ keep,
                                                            int* __restrict__ kept) {
    const int i = blockIdx.x * kPairBlock + threadIdx.x;
    if (i < n_members) mark[i] = alive[i] && grp[group_of[i]].alive >= min_members;
    if (i < n_groups) {
        const int f = grp[i].alive >= min_members;   // (a group that was never stripped below min_members)
        keep[i] = f;
        kept[i] = f ? grp[i].alive : 0;
    }
}

__global__ __launch_bounds__(kPairBlock) void k_unbind_compact(int n_members, const int* __restrict__ members, const int* __restrict__ mark,
                                                               const int* __restrict__ dest, const double* __restrict__ energy,
                                                               int* __restrict__ out_members, double* __restrict__ out_energy) {
    const int i = blockIdx.x * kPairBlock + threadIdx.x;
    if (i >= n_members || !mark[i]) return;
    out_members[dest[i]] = members[i];   // (dest < the reported members <= n_members)
    out_energy[dest[i]] = energy[i];
}

__global__ __launch_bounds__(kPairBlock) void k_unbind_records(int n_groups, const int* __restrict__ size, const int* __restrict__ offset,
                                                               const int* __restrict__ slot_root, const UnbindGroup* __restrict__ grp,
                                                               const int* __restrict__ alive, const double* __restrict__ kinetic,
                                                               const double* __restrict__ potential, const int* __restrict__ keep,
                                                               const int* __restrict__ kept, const int* __restrict__ slot,
                                                               const int* __restrict__ out_offset, NbodyBoundGroup* __restrict__ out,
                                                               int* __restrict__ counters) {
    const int lane = threadIdx.x % 64;
    const int g = blockIdx.x * (kPairBlock / 64) + threadIdx.x / 64;
    if (g >= n_groups) return;   // (wave-uniform)
    if (g == n_groups - 1 && lane == 0) {
        counters[1] = slot[g] + keep[g];
        counters[2] = out_offset[g] + kept[g];
    }
    if (!keep[g]) return;
    const int root = slot_root[g];
    const int off = offset[root], cnt = size[root];
    double s[2] = {0.0, 0.0};
    for (int k = lane; k < cnt; k += 64) {   // seven_sums' shape: lane k mod 64, k the position in the FoF list
        if (!alive[off + k]) continue;
        s[0] += kinetic[off + k];
        s[1] += potential[off + k];
    }
    for (int half = 32; half >= 1; half >>= 1)
        for (int c = 0; c < 2; ++c) s[c] += __shfl_down(s[c], half, 64);
    if (lane) return;
    NbodyBoundGroup r;
    r.first = root;
    r.fof_count = cnt;
    r.count = kept[g];
    r.offset = out_offset[g];
    r.iterations = grp[g].iterations;
    r.converged = grp[g].converged;
    r.mass = grp[g].sum[0];
    for (int c = 0; c < 3; ++c) {
        r.mx[c] = grp[g].sum[1 + c];
        r.mv[c] = grp[g].sum[4 + c];
    }
    r.kinetic = s[0];
    r.potential = s[1];
    out[slot[g]] = r;   // (slot < the reported groups <= n_groups)
}

namespace fof {

namespace {
int waves_grid(int n_groups) { return (n_groups + kPairBlock / 64 - 1) / (kPairBlock / 64); }
UnbindScratch layout(Carver& c, size_t n_members, size_t n_groups) {
    UnbindScratch u;
    u.grp = c.take<UnbindGroup>(n_groups);
    for (int** p : {&u.alive, &u.mark, &u.dest, &u.out_members}) *p = c.take<int>(n_members);
    for (double** p : {&u.energy, &u.kinetic, &u.potential, &u.out_energy}) *p = c.take<double>(n_members);
    for (int** p : {&u.keep, &u.kept, &u.slot, &u.offset}) *p = c.take<int>(n_groups);
    u.out = c.take<NbodyBoundGroup>(n_groups);
    u.counters = c.take<int>(3);
    u.scan_bytes = std::max(pairs::scan_tmp_bytes(n_members), pairs::scan_tmp_bytes(n_groups));
    u.scan_tmp = c.take<char>(u.scan_bytes);
    return u;
}
}  // namespace

size_t unbind_scratch_bytes(size_t n_members, size_t n_groups) { Carver c; layout(c, n_members, n_groups); return c.offset(); }
UnbindScratch unbind_layout(void* base, size_t n_members, size_t n_groups) { Carver c(base); return layout(c, n_members, n_groups); }

void launch_unbind_init(hipStream_t s, int n_members, int n_groups, const FofScratch& w, const UnbindScratch& u) {
    if (n_members <= 0) return;
    hipLaunchKernelGGL(k_unbind_init, dim3(pairs::blocks_for(n_members)), dim3(kPairBlock), 0, s, n_members, n_groups, w.size, w.slot_root,
                       u.grp, u.alive);
}

template <class F>
void launch_unbind_pass(hipStream_t s, const ShardT<F>& sh, int n_upper, int n_members, int n_groups, int min_members, int pass,
                        bool last, double g, double soft2, const FofScratch& w, const UnbindScratch& u) {
    if (n_members <= 0 || n_groups <= 0) return;
    const int* members = w.members(size_t(n_upper));
    const unsigned* group_of = w.keys + n_upper;   // the sorted keys: the group slot of every position of the member list
    hipLaunchKernelGGL(k_unbind_sums<F>, dim3(waves_grid(n_groups)), dim3(kPairBlock), 0, s, sh.own_pos(), sh.vel, n_groups, w.size,
                       w.offset, w.slot_root, members, u.alive, u.grp);
    hipLaunchKernelGGL(k_unbind_energy<F>, dim3(pairs::blocks_for(n_members)), dim3(kPairBlock), 0, s, sh.own_pos(), sh.vel, n_members,
                       w.size, w.offset, w.slot_root, members, group_of, u.grp, u.alive, g, soft2, u.energy, u.kinetic, u.potential,
                       u.mark);
    hipLaunchKernelGGL(k_unbind_verdict, dim3(waves_grid(n_groups)), dim3(kPairBlock), 0, s, n_groups, min_members, pass, int(last),
                       w.size, w.offset, w.slot_root, u.grp, u.alive, u.mark, u.counters);
}

int launch_unbind_finish(hipStream_t s, int n_upper, int n_members, int n_groups, int min_members, const FofScratch& w,
                         const UnbindScratch& u) {
    if (n_members <= 0 || n_groups <= 0) return 0;
    const int* members = w.members(size_t(n_upper));
    const unsigned* group_of = w.keys + n_upper;
    const int blocks = pairs::blocks_for(n_members);
    hipLaunchKernelGGL(k_unbind_keep, dim3(blocks), dim3(kPairBlock), 0, s, n_members, n_groups, min_members, group_of, u.grp, u.alive,
                       u.mark, u.keep, u.kept);
    size_t tb = u.scan_bytes;
    if (rocprim::exclusive_scan(u.scan_tmp, tb, u.mark, u.dest, 0, size_t(n_members), rocprim::plus<int>(), s) != hipSuccess) return -1;
    tb = u.scan_bytes;
    if (rocprim::exclusive_scan(u.scan_tmp, tb, u.keep, u.slot, 0, size_t(n_groups), rocprim::plus<int>(), s) != hipSuccess) return -1;
    tb = u.scan_bytes;
    if (rocprim::exclusive_scan(u.scan_tmp, tb, u.kept, u.offset, 0, size_t(n_groups), rocprim::plus<int>(), s) != hipSuccess) return -1;
    hipLaunchKernelGGL(k_unbind_compact, dim3(blocks), dim3(kPairBlock), 0, s, n_members, members, u.mark, u.dest, u.energy,
                       u.out_members, u.out_energy);
    hipLaunchKernelGGL(k_unbind_records, dim3(waves_grid(n_groups)), dim3(kPairBlock), 0, s, n_groups, w.size, w.offset, w.slot_root,
                       u.grp, u.alive, u.kinetic, u.potential, u.keep, u.kept, u.slot, u.offset, u.out, u.counters);
    return 0;
}

template void launch_unbind_pass<float>(hipStream_t, const ShardT<float>&, int, int, int, int, int, bool, double, double, const FofScratch&,
                                        const UnbindScratch&);
template void launch_unbind_pass<double>(hipStream_t, const ShardT<double>&, int, int, int, int, int, bool, double, double,
                                         const FofScratch&, const UnbindScratch&);

}}  // namespace nbody::fof
