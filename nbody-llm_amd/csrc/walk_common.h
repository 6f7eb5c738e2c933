// walk_common.h -- what the tree walks of kernels_bh.hip, kernels_quad.hip and kernels_f64.hip share: the f32 node record and
// the node-range split with its entry (walk_entry), the monopole coefficient in its three roundings (monopole_k), and the two
// fragments every split walk starts and ends with.  Device code only.
#pragma once
#include "real.h"   // kernels.h (kMaxAnc, NBODY_WALK_COUNTER_SLOTS), Real<F>

namespace nbody {

struct alignas(32) NodeDev { float4 a; float4 b; };  // f32 node record: {com, mass}, {width^2, skip bits, width, leaf body}

// The node index range [0, n_nodes) can be cut into n_seg contiguous segments walked by different
// waves (more waves in flight: at N = 65 536 one wave per 64 bodies is only one wave per SIMD and the
// walk is bound by the latency of its dependent node loads).  A body's walk enters segment k at the
// first node >= first[k] that it would visit: to know, replay the opening tests of the ancestors of
// node first[k] (root first; the host lists them, at most NBODY_MAX_TREE_DEPTH): an accepted
// ancestor's skip link is where the walk resumes.  Ancestors are only tested here -- they are
// counted and accumulated by the segment that contains them -- so every (body, node) pair is
// evaluated by exactly one segment and the counters stay exact.
// (f64 handles: nbody64::WalkSplit64 of kernels_f64.h, the same first four members with double4 planes.)
struct WalkSplit {
    int n_seg;
    const int* first;        // [n_seg + 1] node index where each segment starts; first[n_seg] = n_nodes
    const int* anc;          // [n_seg][kMaxAnc] ancestors of first[k], root first
    const int* n_anc;        // [n_seg]
    float4* planes;          // [n_seg][plane_stride] partial accelerations (n_seg > 1), indexed by the body's place in `order`
                             // (tree order): the walk's lanes and the reduction's both touch consecutive entries
    size_t plane_stride;
    int diag_first;          // k_bh_walk: segments of a body group in order of distance from its own place in the tree
    const int* poison;       // unsynchronised steps: != 0 -> do nothing (Shard::poison); may be null
    const int* n_order_dev;  // unsynchronised steps: the live number of bodies to walk (the host's is an upper bound); may be null
    int store_work;          // k_bh_walk, one segment: the body's visit count goes to acc.w (spatial shards balance by it)
    int xcd_blocks;          // k_bh_walk_duo: gridDim.x / 8 when the lane groups are dealt to the XCDs in eighths of the tree order, else 0
};

// The first node >= first[seg] that the walk of a body at p visits: the opening tests of first[seg]'s ancestors, root first.
// DIRECT = NBODY_LEAF_DIRECT: an ancestor closer than 1e-5 is skipped whole, as the walk itself skips it.
template <bool DIRECT = false>
__device__ __forceinline__ int walk_entry(const NodeDev* __restrict__ nodes, const WalkSplit& sp, int seg,
                                          const float4 p, float theta2) {
    const int s0 = sp.first[seg];
    const int na = sp.n_anc[seg];
    for (int k = 0; k < na; ++k) {
        const int j = sp.anc[seg * kMaxAnc + k];
        const float4 A = nodes[j].a;
        const float4 B = nodes[j].b;
        const float rx = A.x - p.x, ry = A.y - p.y, rz = A.z - p.z;
        const float r2 = (rx * rx + ry * ry) + rz * rz;
        if (DIRECT && r2 < 1e-10f) return __float_as_int(B.y);  // NBODY_LEAF_DIRECT: skipped whole
        if (B.x < theta2 * r2) return __float_as_int(B.y);  // accepted: the walk resumes after its subtree
    }
    return s0;  // every ancestor was opened: the walk arrives at first[seg] itself
}

// g m / r^3 of an accepted monopole, as each force walk rounds it: a = d * monopole_k.
template <bool FAST, bool DIRECT, class F>
__device__ __forceinline__ F monopole_k(F g, F m, F r2, F eps2) {
    if (FAST) {                                        // 1 / sqrt by the hardware's approximation (f32: v_rsq_f32)
        const F rinv = Real<F>::rsqrt(r2 + eps2);
        return (g * m) * ((rinv * rinv) * rinv);
    }
    if (DIRECT) {
        const F inv_r = F(1) / Real<F>::sqrt(r2 + eps2);   // llm :942
        const F inv_r3 = inv_r * inv_r * inv_r;            // llm :944
        return g * m * inv_r3;                             // llm :947
    }
    const F r_dist = Real<F>::sqrt(r2 + eps2);         // :193
    const F r_cubed = r_dist * r_dist * r_dist;        // :194
    return ((g * m) / r_cubed);                        // :195
}

// Which of the K node-range segments workgroup (bx of gx, blockIdx.y = kk) walks.  The launch lasts as long as its slowest
// wave, and a body group's long walks are in the segments around its own place in the tree (that is where cells are opened
// down to the leaves).  Bodies are in tree order, so group bx of gx sits near node bx/gx * n_nodes: the segments are taken
// by distance from that "diagonal" -- kk = 0 is the group's own segment, then +1, -1, +2, ... -- and the dispatcher, which
// hands out workgroups in blockIdx order (x fastest), starts the heavy ones first.
// (Index: unsigned for blockIdx.x itself, int for a remapped one -- the 64-bit product is formed from it as it comes.)
template <class Index>
__device__ __forceinline__ int nearest_first_segment(Index bx, unsigned gx, int kk, int K) {
    const int diag = int((long long)bx * K / gx);
    const int off = (kk & 1) ? (kk + 1) / 2 : -(kk / 2);
    return ((diag + off) % K + K) % K;
}

// The lanes' {accepted, visited} counts added up over the wave and into pair `slot` (taken modulo the slot count) of
// `counters` (may be null): one atomic pair per wave, spread over NBODY_WALK_COUNTER_SLOTS address pairs -- 16 384 atomics
// on ONE address pair serialise in L2 at ~13 ns each (0.21 ms per walk at 8 segments, measured with theta2 = 1e9).
// Called by every lane of the wave, outside divergent code.
__device__ __forceinline__ void add_walk_counts(unsigned long long* __restrict__ counters, unsigned slot, unsigned int n_acc,
                                                unsigned int n_vis) {
    for (int off = 32; off > 0; off >>= 1) {
        n_acc += __shfl_down(n_acc, off);
        n_vis += __shfl_down(n_vis, off);
    }
    if ((threadIdx.x & 63) == 0 && counters) {
        slot &= NBODY_WALK_COUNTER_SLOTS - 1;
        atomicAdd(&counters[2 * slot], (unsigned long long)n_acc);
        atomicAdd(&counters[2 * slot + 1], (unsigned long long)n_vis);
    }
}

}  // namespace nbody
