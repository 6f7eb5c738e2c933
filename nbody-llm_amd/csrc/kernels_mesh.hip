// kernels_mesh.hip -- the last stage of a mesh-gravity pass on the device (gfx950; include/nbody_hip.h, "mesh gravity").
// Compiled with -ffp-contract=off.  The deposit, the solve and the orders are kernels_deposit.hip's, kernels_poisson.hip's and
// kernels_sample.hip's launches as they stand; what is new is
//
//   k_mesh_kick<F, kReach, kScheme>  one lane per place of the home-cell order (or per row, unsorted).  The stencil set-up
//                   and the gradient are sample_device.h's LaneStencil and lane_gradient: the gradient_component<K> calls of
//                   k_sample and k_pm_gather, so every component is those kernels' expression tree.  No phi sum, no class, no
//                   count and no f64 row: the lane forms 0.0 - grad, rounds it ONCE to F and stores {ax, ay, az, 0} in the
//                   shard's acc row; with a
//                   kick it then applies real.h's kick_half_drift to its own row.  A lane touches its own row only, the grid is
//                   read-only here, so the order of the lanes changes nothing.  No LDS, no floating-point atomics, no lane waits
//                   for another.  256 lanes a block, as the gathers: neighbours in home-cell order read neighbouring cells.
//   k_mesh_round<F> mesh_kick_fuse = 0: the f64 rows of the gather become the acc rows, rounded once
#include "kernels_mesh.h"
#include "sample_device.h"
#include "kernels.h"   // tuning()
#include "real.h"      // kick_half_drift

namespace nbody {

using sample::kSampleBlock;

template <class F, int kReach, int kScheme>
__global__ __launch_bounds__(kSampleBlock) void k_mesh_kick(const double* __restrict__ xyz, const int* __restrict__ count, int n, deposit::Grid g,
                                                            double den, const double* __restrict__ G, const int* __restrict__ rows,
                                                            typename Real<F>::V4* __restrict__ pos, typename Real<F>::V4* __restrict__ vel,
                                                            typename Real<F>::V4* __restrict__ acc, int kick, F dt) {
    constexpr int kCnt = kScheme + 1;
    sample::LaneStencil<kCnt> lane;
    lane.set_up(xyz, count, n, g, kReach, rows, blockIdx.x * kSampleBlock + threadIdx.x);
    unsigned long long reads = 0;   // (lane_gradient counts them; nobody reads the count here)
    double grad[3];
    sample::lane_gradient<kCnt, kReach>(g, G, lane, den, reads, grad);
    const int row = lane.row;   // (< the live count, which is <= n <= the shard's capacity)
    if (row < 0) return;
    const F ax = F(0.0 - grad[0]), ay = F(0.0 - grad[1]), az = F(0.0 - grad[2]);
    acc[row] = Real<F>::make4(ax, ay, az, F(0));
    if (kick) kick_half_drift(pos, vel, row, ax, ay, az, dt);
}

template <class F>
__global__ __launch_bounds__(kSampleBlock) void k_mesh_round(const int* __restrict__ count, int n, const double* __restrict__ rows3,
                                                             typename Real<F>::V4* __restrict__ acc) {
    const int i = blockIdx.x * kSampleBlock + threadIdx.x;
    if (i >= live_count(count, n)) return;
    acc[i] = Real<F>::make4(F(rows3[3 * size_t(i)]), F(rows3[3 * size_t(i) + 1]), F(rows3[3 * size_t(i) + 2]), F(0));
}

namespace mesh {

Plan make_plan() {
    const Tuning& t = nbody::tuning();
    Plan p;
    p.kick_fuse = t.mesh_kick_fuse != 0;
    p.keep_kernel = t.mesh_keep_kernel != 0;
    return p;
}

template <class F>
void launch_kick(hipStream_t s, const ShardT<F>& sh, const int* count, int n, const deposit::Grid& g, int gradient_op, const int* rows,
                 const pm::Scratch& w, const F* kick_dt) {
    if (n <= 0) return;
    const dim3 grid(sample::blocks_for(size_t(n))), block(kSampleBlock);
    const double den = sample::denominator_of(gradient_op, g.spacing);
    const int kick = kick_dt ? 1 : 0;
    const F dt = kick_dt ? *kick_dt : F(0);
    sample::for_reach_and_scheme(gradient_op, g.scheme, [&](auto reach, auto scheme) {
        hipLaunchKernelGGL((k_mesh_kick<F, decltype(reach)::value, decltype(scheme)::value>), grid, block, 0, s, w.smp.xyz, count, n, g, den, w.smp.grid,
                           rows, sh.own_pos(), sh.vel, sh.acc, kick, dt);
    });
}

template <class F>
void launch_round(hipStream_t s, const ShardT<F>& sh, const int* count, int n, const double* rows3) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_mesh_round<F>, dim3(sample::blocks_for(size_t(n))), dim3(kSampleBlock), 0, s, count, n, rows3, sh.acc);
}

template void launch_kick<float>(hipStream_t, const ShardT<float>&, const int*, int, const deposit::Grid&, int, const int*, const pm::Scratch&, const float*);
template void launch_kick<double>(hipStream_t, const ShardT<double>&, const int*, int, const deposit::Grid&, int, const int*, const pm::Scratch&,
                                  const double*);
template void launch_round<float>(hipStream_t, const ShardT<float>&, const int*, int, const double*);
template void launch_round<double>(hipStream_t, const ShardT<double>&, const int*, int, const double*);

}}  // namespace nbody::mesh
