// kernels_pot.h -- launchers behind nbody_potentials / nbody_energy_world (internal to libnbody_hip.so): the potential
// walks (kernels_bh.hip, kernels_f64.hip) and the exact pair sums and energy partials (kernels_pot.hip).  All of them
// leave S_i = sum_j m_j / sqrt(|x_j - x_i|^2 + eps2) per own body in an f64 array indexed like the own segment; the host
// multiplies by -g.
#pragma once
#include "kernels.h"
#include "kernels_f64.h"

namespace nbody {

// the bodies of a handle of either dtype as the pair kernels read them: every segment's {x, y, z, m} and live count
struct PotBodies {
    const void* pos_all = nullptr;   // float4 (f64 = 0) or double4 (f64 = 1) [n_seg][seg_cap]
    const void* vel = nullptr;       // own segment's velocities, the same element type
    const int* seg_count = nullptr;
    int f64 = 0, n_seg = 1, seg_cap = 0, my_seg = 0;
    int world = 1;                   // ranks whose energies nbody_energy_world adds up (index blocks: n_seg; spatial shards: the world)
};

// NBODY_POTENTIAL_TREE, f32 handles: t = the force pass's tree, order and split view (its planes and counters are not used)
void launch_bh_pot_walk(hipStream_t s, const float4* own_pos, const TreeDev& t, float g_soft2, float theta2, double* planes,
                        size_t plane_stride, double* sum, unsigned long long* counters /* [NBODY_WALK_COUNTER_SLOTS][2] */);
void launch_pot_reduce(hipStream_t s, const double* planes, int n_seg, size_t plane_stride, const int* order, int n_order, double* sum,
                       const int* n_order_dev = nullptr /* device: the live number of bodies (n_order is then an upper bound) */);

// NBODY_POTENTIAL_PAIRS: coordinate differences, terms and sums in f64 (exact differences for f32 bodies), IEEE sqrt and
// divide.  p = make_bf64_plan's shape for the own block (kernels_bf64.hip): from Tuning::bf64_min_bodies bodies every
// unordered pair of the own block once (resident sets in registers, travelling chunks, k_pot_sym) and the pairs it leaves
// over one-sided; below, one-sided tiles alone; the other index blocks' bodies one-sided.  planes: p.n_planes * p.n_pad
// doubles, every row written once, added in plane order.
void launch_pot_pairs(hipStream_t s, const PotBodies& b, const nbody64::Bf64Plan& p, double* planes, double eps2, int n_upper, double* sum);

// Spatial shards: the sums come back from the ranks that walked the bodies (a scratch world in which strayed bodies have
// migrated) to the ranks that own them.  A record per walked body, all-gathered in slots of seg_cap records per rank; the
// owner finds its bodies by their index in the uploaded vector.
struct PotRec { int id; int pad; double sum; };
void launch_pot_pack(hipStream_t s, const int* ids, const double* sum, const int* count, int n_upper, PotRec* out);
// slot_of [n_ids] must hold -1; own_ids [*own_count] = the owner's bodies; rec [world][seg_cap], rec_count [world]
void launch_pot_scatter(hipStream_t s, const int* own_ids, const int* own_count, int own_upper, int* slot_of, int n_ids, const PotRec* rec,
                        const int* rec_count, int world, int seg_cap, double* sum);

// per 256-body block {sum 1/2 m v^2, sum m_i S_i}, the block's terms added in a fixed tree order; out2: 2 doubles per block
void launch_pot_energy(hipStream_t s, const PotBodies& b, const double* sum, int n_upper, double* out2);

}  // namespace nbody

namespace nbody64 {
// NBODY_POTENTIAL_TREE, f64 handles; the caller adds the planes with nbody::launch_pot_reduce
void launch_bh_pot_walk(hipStream_t s, const double4* pos, const Node64* nodes, const int* order, int n_order, double eps2, double theta2,
                        const WalkSplit64& split, double* planes, size_t plane_stride, unsigned long long* counters);
}  // namespace nbody64
