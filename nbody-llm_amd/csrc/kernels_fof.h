// kernels_fof.h -- launchers of the friends-of-friends group finder (kernels_fof.hip): the connected components of "closer
// than a linking length" over all pairs, every body's label (the lowest index of its component), and the catalogue of the
// components with at least min_members bodies.  Internal to libnbody_hip.so.
#pragma once
#include "nbody_hip.h"      // NbodyGroup
#include "kernels_pairs.h"  // PartnerPlan, kPairBlock: k_fof_link runs on k_partner's frame
#include "shard.h"
#if defined(__HIPCC__)
#include "real.h"           // widen
#endif

namespace nbody { namespace fof {

#if defined(__HIPCC__)
// ---- what every link pass shares on the device (k_fof_link; k_cells_link of kernels_cells.hip)
// parent[] in global memory under the three operations of fof_union.h
struct DevParent {
    int* p;
    __device__ __forceinline__ int load(int x) const { return __hip_atomic_load(p + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ int cas(int x, int expect, int want) const { return atomicCAS(p + x, expect, want); }
    __device__ __forceinline__ void lower(int x, int v) const { atomicMin(p + x, v); }
};

// r2_ij = (dx dx + dy dy) + dz dz, unsoftened (nbody_nearest's metric): r2_ij == r2_ji bit for bit
__device__ __forceinline__ double pair_dist2(const double4 pi, const double4 pj) {
    const double dx = pj.x - pi.x, dy = pj.y - pi.y, dz = pj.z - pi.z;
    return (dx * dx + dy * dy) + dz * dz;
}

// THE SEVEN SUMS of one group in the header's order, by one wave: who[k], k = 0 .. cnt-1, are its members in ascending index;
// lane t = k mod 64 adds its terms in ascending k from +0.0 -- m, m x_c, m v_c, each product rounded once -- then sum[t] +=
// sum[t + half] for half = 32, 16, ... 1: lane 0 holds the result.  alive (may be nullptr: everybody) is parallel to who: a
// member whose flag is 0 adds nothing, and k stays its position in who (k_fof_sums; k_unbind_sums of kernels_unbind.hip).
template <class F>
__device__ __forceinline__ void seven_sums(const typename Real<F>::V4* __restrict__ pos, const typename Real<F>::V4* __restrict__ vel,
                                           const int* __restrict__ who, int cnt, const int* __restrict__ alive, int lane, double s[7]) {
    for (int c = 0; c < 7; ++c) s[c] = 0.0;
    for (int k = lane; k < cnt; k += 64) {
        if (alive && !alive[k]) continue;
        const int b = who[k];
        const double4 p = widen(pos[b]), v = widen(vel[b]);
        s[0] += p.w;
        s[1] += p.w * p.x;
        s[2] += p.w * p.y;
        s[3] += p.w * p.z;
        s[4] += p.w * v.x;
        s[5] += p.w * v.y;
        s[6] += p.w * v.z;
    }
    for (int half = 32; half >= 1; half >>= 1)
        for (int c = 0; c < 7; ++c) s[c] += __shfl_down(s[c], half, 64);   // (lanes >= half carry sums nobody reads)
}
#endif

// The scratch of one call for n_upper rows, carved out of one allocation of scratch_bytes.
struct FofScratch {
    int* parent = nullptr;      // [n_upper] the union-find forest (-1 past the live count); dead after k_fof_flatten
    int* label = nullptr;       // [n_upper] the root of a live row = the lowest index of its component (-1 past the live count)
    int* size = nullptr;        // [n_upper] members of the component whose root the row is, else 0
    int* flag = nullptr;        // [n_upper] 1 = a root with size >= min_members: a listed group
    int* listed = nullptr;      // [n_upper] size where flag, else 0
    int* slot = nullptr;        // [n_upper] exclusive prefix sums of flag: the group's place in the catalogue
    int* offset = nullptr;      // [n_upper] exclusive prefix sums of listed: of the group's members in the member list
    int* slot_root = nullptr;   // [n_upper] the root of the group in each slot
    unsigned* keys = nullptr;   // [2 n_upper] a row's group slot, or INT_MAX when its component is not listed; in | out
    int* rows = nullptr;        // [2 n_upper] the row index; in | out: out = the member list, then everybody else
    int* total = nullptr;       // [2] listed groups, their members
    void* scan_tmp = nullptr;
    size_t scan_bytes = 0;
    void* sort_tmp = nullptr;
    size_t sort_bytes = 0;
    const int* members(size_t n_upper) const { return rows + n_upper; }
};
size_t scratch_bytes(size_t n_upper);
FofScratch scratch_layout(void* base, size_t n_upper);

// k_fof_init, k_fof_link<F> on the grid of `p`, k_fof_flatten: w.label and w.size of the live rows for the links r2 < B2
template <class F>
void launch_components(hipStream_t s, const ShardT<F>& sh, int n_upper, const pairs::PartnerPlan& p, double B2, const FofScratch& w);
// its first and last launch alone, for a link pass of another kind between them (kernels_cells.hip)
void launch_forest_init(hipStream_t s, const int* count, int n_upper, const FofScratch& w);
void launch_flatten(hipStream_t s, const int* count, int n_upper, const FofScratch& w);

// k_fof_flag, the two integer scans, k_fof_slots: w.flag, w.slot, w.offset, w.slot_root, w.keys and w.total; `sort`: the
// stable radix sort of (slot, row) after them: w.members().  Returns 0, or -1 when a rocPRIM call could not be enqueued.
int launch_catalogue(hipStream_t s, int n_upper, int min_members, bool sort, const FofScratch& w);

// k_fof_sums<F>, one wave per listed group: out[0 .. n_groups), every field (out: device memory)
template <class F>
void launch_sums(hipStream_t s, const ShardT<F>& sh, int n_upper, int n_groups, const FofScratch& w, NbodyGroup* out);

}}  // namespace nbody::fof
