// kernels_integrate.hip -- O(N) kernels around the force pass (gfx950), written once for F = f32 and F = f64 (real.h)
// with their launchers over ShardT<F> (kernels.h).
//
// K0  AoS <-> SoA transposition of PointParticle<F,3> records (shared.rs:151-158)
// K1  drift_half    = LeapFrogIntegrator::integrate_pre_force (shared.rs:135-140)
//                     + the Bounds::contains test (shared.rs:210-212) that retain() applies next
// K4  compact       = Vec::retain (brute_force.rs:86, barnes_hut.rs:267), order preserving, one pass over many workgroups:
//                     the look-back scan is retain.h's, here is what moves with a leapfrog body
// K3  kick_drift    = LeapFrogIntegrator::integrate_after_force (shared.rs:141-148)
//
// All are pure streaming kernels, 16 B (f32) or 32 B (f64) per lane per access.
// Compiled with -ffp-contract=off: (v*0.5)*dt and a*dt are rounded products, then added, exactly
// as the reference's nalgebra expressions evaluate.
#include "real.h"
#include "retain.h"

#include <algorithm>

namespace nbody {

// F = float: the f32 handles (poison: Shard::poison, may be null); F = double: the f64 handles (poison and ids null)
template <class F>
__global__ __launch_bounds__(256) void k_aos_to_soa(const F* __restrict__ aos, int stride, int n, typename Real<F>::V4* __restrict__ pos,
                                                    typename Real<F>::V4* __restrict__ vel, typename Real<F>::V4* __restrict__ acc) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const F* p = aos + size_t(k) * stride;
    pos[k] = Real<F>::make4(p[0], p[1], p[2], p[9]);
    if (vel) vel[k] = Real<F>::make4(p[3], p[4], p[5], F(0));  // other shards' segments carry positions only
    if (acc) acc[k] = Real<F>::make4(p[6], p[7], p[8], F(0));
}

template <class F>
__global__ __launch_bounds__(256) void k_soa_to_aos(F* __restrict__ aos, int stride, int n, const typename Real<F>::V4* __restrict__ pos,
                                                    const typename Real<F>::V4* __restrict__ vel,
                                                    const typename Real<F>::V4* __restrict__ acc) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const typename Real<F>::V4 p = pos[k], v = vel[k], a = acc[k];
    F* o = aos + size_t(k) * stride;
    o[0] = p.x; o[1] = p.y; o[2] = p.z;
    o[3] = v.x; o[4] = v.y; o[5] = v.z;
    o[6] = a.x; o[7] = a.y; o[8] = a.z;
    o[9] = p.w;
}

template <class F>
__global__ __launch_bounds__(256) void k_drift_half(typename Real<F>::V4* __restrict__ pos, const typename Real<F>::V4* __restrict__ vel,
                                                    const int* __restrict__ count, unsigned char* __restrict__ keep,
                                                    int* __restrict__ escaped, F dt, typename Real<F>::Bounds b,
                                                    const int* __restrict__ poison) {
    if (poison && *poison) return;
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= *count) return;
    typename Real<F>::V4 p = pos[k];
    const typename Real<F>::V4 v = vel[k];
    p.x += (v.x * Real<F>::half) * dt;
    p.y += (v.y * Real<F>::half) * dt;
    p.z += (v.z * Real<F>::half) * dt;
    pos[k] = p;
    // inclusive, component-wise; a NaN fails every comparison and is dropped
    const bool in = (p.x >= b.lo[0]) && (p.x <= b.hi[0]) && (p.y >= b.lo[1]) && (p.y <= b.hi[1]) &&
                    (p.z >= b.lo[2]) && (p.z <= b.hi[2]);
    keep[k] = in ? 1 : 0;
    if (!in) atomicAdd(escaped, 1);
}

template <class F>
__global__ __launch_bounds__(256) void k_kick_drift(typename Real<F>::V4* __restrict__ pos, typename Real<F>::V4* __restrict__ vel,
                                                    const typename Real<F>::V4* __restrict__ acc, const int* __restrict__ count,
                                                    F dt, int* __restrict__ poison) {
    if (poison && *poison) return;
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k == 0 && poison) atomicAdd(poison + 1, 1);   // a step of an unsynchronised Barnes-Hut run is complete
    if (k >= *count) return;
    typename Real<F>::V4 p = pos[k], v = vel[k];
    const typename Real<F>::V4 a = acc[k];
    v.x += a.x * dt;
    v.y += a.y * dt;
    v.z += a.z * dt;
    p.x += (v.x * Real<F>::half) * dt;
    p.y += (v.y * Real<F>::half) * dt;
    p.z += (v.z * Real<F>::half) * dt;
    vel[k] = v;
    pos[k] = p;
}

// K4: retain.h's look-back scan; what moves with a leapfrog body is three arrays and, on spatial shards, its id (else null)
template <class F>
__global__ __launch_bounds__(kCompactTile) void k_compact(typename Real<F>::V4* __restrict__ pos, typename Real<F>::V4* __restrict__ vel,
                                                          typename Real<F>::V4* __restrict__ acc, const unsigned char* __restrict__ keep,
                                                          int* __restrict__ count, int* __restrict__ escaped,
                                                          unsigned long long* __restrict__ tile_state, int* __restrict__ epoch_p,
                                                          const int* __restrict__ poison, int* __restrict__ ids) {
    if (poison && *poison) return;
    if (*escaped == 0) return;
    typename Real<F>::V4 p = Real<F>::make4(0, 0, 0, 0), v = p, a = p;
    int id = 0;
    retain_tile(keep, count, escaped, tile_state, epoch_p,
                [&](int k) { p = pos[k]; v = vel[k]; a = acc[k]; if (ids) id = ids[k]; },
                [&](int d) { pos[d] = p; vel[d] = v; acc[d] = a; if (ids) ids[d] = id; });
}

static inline int blocks_for(int n, int bs) { return n <= 0 ? 0 : (n + bs - 1) / bs; }

template <class F>
void launch_aos_to_soa(hipStream_t s, const F* aos, int stride, int n, typename ShardT<F>::V4* pos, typename ShardT<F>::V4* vel,
                       typename ShardT<F>::V4* acc) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_aos_to_soa<F>, dim3(blocks_for(n, 256)), dim3(256), 0, s, aos, stride, n, pos, vel, acc);
}
template <class F>
void launch_soa_to_aos(hipStream_t s, F* aos, int stride, int n, const typename ShardT<F>::V4* pos, const typename ShardT<F>::V4* vel,
                       const typename ShardT<F>::V4* acc) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_soa_to_aos<F>, dim3(blocks_for(n, 256)), dim3(256), 0, s, aos, stride, n, pos, vel, acc);
}
template <class F>
void launch_drift_half(hipStream_t s, const ShardT<F>& sh, int n_upper, F dt, const typename RealTypes<F>::Bounds& b) {
    if (n_upper <= 0) return;
    hipLaunchKernelGGL(k_drift_half<F>, dim3(blocks_for(n_upper, 256)), dim3(256), 0, s, sh.own_pos(), sh.vel, sh.own_count(), sh.keep,
                       sh.escaped, dt, b, sh.poison);
}
template <class F>
void launch_compact(hipStream_t s, const ShardT<F>& sh, int n_upper) {
    if (n_upper <= 0) return;
    hipLaunchKernelGGL(k_compact<F>, dim3(blocks_for(n_upper, kCompactTile)), dim3(kCompactTile), 0, s, sh.own_pos(), sh.vel, sh.acc,
                       sh.keep, sh.own_count(), sh.escaped, sh.tile_state, sh.epoch, sh.poison, sh.ids);
}
template <class F>
void launch_kick_drift(hipStream_t s, const ShardT<F>& sh, int n_upper, F dt) {
    // with a poison word even an empty shard launches one block: the step counter of an unsynchronised run rides in it
    const int blocks = blocks_for(n_upper, 256);
    if (blocks == 0 && !sh.poison) return;
    hipLaunchKernelGGL(k_kick_drift<F>, dim3(std::max(1, blocks)), dim3(256), 0, s, sh.own_pos(), sh.vel, sh.acc, sh.own_count(), dt,
                       sh.poison);
}

#define NBODY_INTEGRATE_LAUNCHERS(F, V4)                                                                              \
    template void launch_aos_to_soa<F>(hipStream_t, const F*, int, int, V4*, V4*, V4*);                               \
    template void launch_soa_to_aos<F>(hipStream_t, F*, int, int, const V4*, const V4*, const V4*);                   \
    template void launch_drift_half<F>(hipStream_t, const ShardT<F>&, int, F, const RealTypes<F>::Bounds&);           \
    template void launch_compact<F>(hipStream_t, const ShardT<F>&, int);                                              \
    template void launch_kick_drift<F>(hipStream_t, const ShardT<F>&, int, F);
NBODY_INTEGRATE_LAUNCHERS(float, float4)
NBODY_INTEGRATE_LAUNCHERS(double, double4)
#undef NBODY_INTEGRATE_LAUNCHERS

}  // namespace nbody

namespace nbody64 {
void launch_aos_to_pos(hipStream_t s, const double* aos, int stride_d, int n, double4* pos) {   // another shard's block: positions only
    nbody::launch_aos_to_soa<double>(s, aos, stride_d, n, pos, nullptr, nullptr);
}
}  // namespace nbody64
