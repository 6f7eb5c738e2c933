// kernels_integrate.hip -- O(N) kernels around the force pass (gfx950), written once for F = f32 and F = f64 (real.h)
// with the launchers of both (kernels.h, kernels_f64.h).
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

// F = float: the f32 handles (poison: Shard::poison, may be null); F = double: the f64 handles (nbody64, no poison)
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

void launch_aos_to_soa(hipStream_t s, const float* aos, int stride_f, int n, float4* pos, float4* vel, float4* acc) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_aos_to_soa<float>, dim3(blocks_for(n, 256)), dim3(256), 0, s, aos, stride_f, n, pos, vel, acc);
}
void launch_soa_to_aos(hipStream_t s, float* aos, int stride_f, int n, const float4* pos, const float4* vel, const float4* acc) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_soa_to_aos<float>, dim3(blocks_for(n, 256)), dim3(256), 0, s, aos, stride_f, n, pos, vel, acc);
}
void launch_drift_half(hipStream_t s, const Shard& sh, int n_upper, float dt, BoundsF b) {
    if (n_upper <= 0) return;
    hipLaunchKernelGGL(k_drift_half<float>, dim3(blocks_for(n_upper, 256)), dim3(256), 0, s, sh.own_pos(), sh.vel,
                       sh.own_count(), sh.keep, sh.escaped, dt, b, sh.poison);
}
void launch_compact(hipStream_t s, const Shard& sh, int n_upper) {
    if (n_upper <= 0) return;
    hipLaunchKernelGGL(k_compact<float>, dim3(blocks_for(n_upper, kCompactTile)), dim3(kCompactTile), 0, s, sh.own_pos(), sh.vel, sh.acc,
                       sh.keep, sh.own_count(), sh.escaped, sh.tile_state, sh.epoch, sh.poison, sh.ids);
}
void launch_kick_drift(hipStream_t s, const Shard& sh, int n_upper, float dt) {
    // (launched even for an empty shard: the step counter of an unsynchronised run rides in it)
    hipLaunchKernelGGL(k_kick_drift<float>, dim3(std::max(1, blocks_for(n_upper, 256))), dim3(256), 0, s, sh.own_pos(), sh.vel, sh.acc,
                       sh.own_count(), dt, sh.poison);
}

}  // namespace nbody

// F = f64 (kernels_f64.h): one shard's own block, no poison word; an empty block launches nothing
namespace nbody64 {
using nbody::blocks_for;

void launch_aos_to_soa(hipStream_t s, const double* aos, int stride_d, int n, const Dev& d, size_t first) {
    if (n <= 0) return;
    hipLaunchKernelGGL(nbody::k_aos_to_soa<double>, dim3(blocks_for(n, 256)), dim3(256), 0, s, aos, stride_d, n, d.pos + first, d.vel + first,
                       d.acc + first);
}
void launch_aos_to_pos(hipStream_t s, const double* aos, int stride_d, int n, double4* pos) {   // another shard's block: positions only
    if (n <= 0) return;
    hipLaunchKernelGGL(nbody::k_aos_to_soa<double>, dim3(blocks_for(n, 256)), dim3(256), 0, s, aos, stride_d, n, pos, (double4*)nullptr,
                       (double4*)nullptr);
}
void launch_soa_to_aos(hipStream_t s, double* aos, int stride_d, int n, const Dev& d) {
    if (n <= 0) return;
    hipLaunchKernelGGL(nbody::k_soa_to_aos<double>, dim3(blocks_for(n, 256)), dim3(256), 0, s, aos, stride_d, n, d.pos, d.vel, d.acc);
}
void launch_drift_half(hipStream_t s, const Dev& d, int n_upper, double dt, const Bounds64& b) {
    if (n_upper <= 0) return;
    hipLaunchKernelGGL(nbody::k_drift_half<double>, dim3(blocks_for(n_upper, 256)), dim3(256), 0, s, d.pos, d.vel, d.count, d.keep, d.escaped, dt,
                       b, (const int*)nullptr);
}
void launch_compact(hipStream_t s, const Dev& d, int n_upper) {
    if (n_upper <= 0) return;
    hipLaunchKernelGGL(nbody::k_compact<double>, dim3(blocks_for(n_upper, nbody::kCompactTile)), dim3(nbody::kCompactTile), 0, s, d.pos, d.vel,
                       d.acc, d.keep, d.count, d.escaped, d.tile_state, d.epoch, (const int*)nullptr, (int*)nullptr);
}
void launch_kick_drift(hipStream_t s, const Dev& d, int n_upper, double dt) {
    if (n_upper <= 0) return;
    hipLaunchKernelGGL(nbody::k_kick_drift<double>, dim3(blocks_for(n_upper, 256)), dim3(256), 0, s, d.pos, d.vel, d.acc, d.count, dt,
                       (int*)nullptr);
}

}  // namespace nbody64
