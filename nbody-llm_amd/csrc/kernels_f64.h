// kernels_f64.h -- launchers of the F = f64 kernels (internal to libnbody_hip.so); see kernels_f64.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "shard.h"

#ifndef NBODY_WALK_COUNTER_SLOTS
#define NBODY_WALK_COUNTER_SLOTS 1024u
#endif

namespace nbody64 {

// one node of the linearised octree: NodeRecT<double> of octree_host.h (64 bytes)
struct alignas(64) Node64 {
    double x, y, z, m;   // centre of mass, mass
    double w2;           // width^2
    int skip, hot, body, pad;
    double pad2;
};
static_assert(sizeof(Node64) == 64, "Node64 layout");

struct alignas(32) Open64 { double x, y, z; int end; int pad; };   // an open cell of the nested walk: its partial sum and where it ends

// K0-K4 are kernels.h's launch_*<double> over Dev = ShardT<double> (shard.h)
void launch_aos_to_pos(hipStream_t s, const double* aos, int stride_d, int n, double4* pos);   // another shard's block: positions only
void launch_bf_strict(hipStream_t s, const Dev& d, int n_upper, double g, double eps2);
void launch_bh_walk(hipStream_t s, const Dev& d, const Node64* nodes, int n_nodes, const int* order, int n_order, double g, double eps2,
                    double theta2, unsigned long long* counters, int leaf_direct, Open64* stack, size_t stack_stride);
// fast f64 walk (NBODY_MATH_FAST on an f64 handle): one running sum per lane instead of the reference's nested sums,
// rsqrt + FMA instead of sqrt and divide, and the node index range cut into n_seg segments walked by different waves
// (walk_common.h WalkSplit: a body's walk enters segment k where the replay of the opening tests of first[k]'s
// ancestors says it would); the K partial sums are added in segment order by launch_bh_reduce64.
struct WalkSplit64 {
    int n_seg;
    const int* first;      // [n_seg + 1]
    const int* anc;        // [n_seg][nbody::kMaxAnc] (kernels.h)
    const int* n_anc;      // [n_seg]
    double4* planes;       // [n_seg][plane_stride], by tree-order position
    size_t plane_stride;
};
void launch_bh_walk_fast(hipStream_t s, const Dev& d, const Node64* nodes, int n_nodes, const int* order, int n_order, double g, double eps2,
                         double theta2, unsigned long long* counters, int leaf_direct, const WalkSplit64& split, int bodies_per_lane = 1,
                         const double* kick_dt = nullptr /* fuse integrate_after_force into the plane reduction */, int* kicked = nullptr);
void launch_energy(hipStream_t s, const Dev& d, int n_upper, double eps2, double* out2);

// fast brute force (NBODY_MATH_FAST on an f64 handle, kernels_bf64.hip).  Planes of double4[n_pad]: [0, sym_sets) the
// travelling-side sums of set distance d, [sym_sets, sym_sets + K) the resident-side sums of slice k, then k_own slices of
// the one-sided own-block pairs, then k_remote slices of the other blocks' bodies; every row is written once a pass.
constexpr int kBf64SmallIptBelow = 16384;   // up to this many bodies k_bf64_sym keeps 4 bodies per lane, beyond it 8
struct Bf64Plan {
    bool sym = false;       // k_bf64_sym + the left-over pairs (else k_bf64_os over every own pair)
    int ipt = 0, rot = 0;   // bodies per lane of a resident set; rotation scheme (Tuning::bf64_rot)
    int A = 0, sym_sets = 0, K = 0;
    int groups = 0;         // 64-body groups of the padded own block
    int k_own = 0, k_remote = 0;
    int n_planes = 0;
    size_t n_pad = 0;
};
Bf64Plan make_bf64_plan(int n_upper, int n_remote_upper, int n_seg, int force_ipt = 0 /* != 0: this many bodies per lane whatever bf64_ipt says (kernels_hermite.h) */);
uint64_t bf64_sym_pairs(const Bf64Plan& p, size_t n);   // unordered pairs of real bodies k_bf64_sym evaluates
void launch_bf64_sym(hipStream_t s, const Dev& d, const Bf64Plan& p, double4* planes, double eps2);
void launch_bf64_own(hipStream_t s, const Dev& d, const Bf64Plan& p, double4* planes, double eps2);      // left-over (or all) own pairs
void launch_bf64_remote(hipStream_t s, const Dev& d, const Bf64Plan& p, double4* planes, double eps2);   // the other blocks' bodies
void launch_bf64_reduce(hipStream_t s, const Dev& d, const Bf64Plan& p, const double4* planes, int n_upper, double g,
                        const double* kick_dt /* != nullptr: integrate_after_force rides along */);

}  // namespace nbody64
