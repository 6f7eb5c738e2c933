// real.h -- what the kernels written once for F = f32 and F = f64 need to know about the real type (the reference's
// trait is generic over Float, shared.rs:12-44): K0, K1, K3, K4 (kernels_integrate.hip), K2 strict (kernels_bf.hip) and the
// tree traversal (walk_common.h); and the two per-particle fragments that come in both types, widen() and kick_half_drift().
#pragma once
#include "kernels.h"
#include "kernels_f64.h"

namespace nbody {

template <class F> struct Real;   // RealTypes<F> (shard.h: V4, Bounds) + the arithmetic only device code can name
template <> struct Real<float> : RealTypes<float> {
    static constexpr float half = 0.5f;
    static __device__ __forceinline__ V4 make4(float x, float y, float z, float w) { return make_float4(x, y, z, w); }
    static __device__ __forceinline__ float sqrt(float x) { return __builtin_sqrtf(x); }   // IEEE (-fhip-fp32-correctly-rounded-divide-sqrt)
    static __device__ __forceinline__ float rsqrt(float x) { return __builtin_amdgcn_rsqf(x); }   // fast math: v_rsq_f32, 1 ulp
};
template <> struct Real<double> : RealTypes<double> {
    static constexpr double half = 0.5;
    static __device__ __forceinline__ V4 make4(double x, double y, double z, double w) { return make_double4(x, y, z, w); }
    static __device__ __forceinline__ double sqrt(double x) { return __builtin_sqrt(x); }  // correctly rounded on gfx950
    static __device__ __forceinline__ double rsqrt(double x) { return ::rsqrt(x); }        // fast math: the device library's
};

// a {x, y, z, w} of either type in f64 (exact)
__device__ __forceinline__ double4 widen(const double4 p) { return p; }
__device__ __forceinline__ double4 widen(const float4 p) { return make_double4(double(p.x), double(p.y), double(p.z), double(p.w)); }

// LeapFrogIntegrator::integrate_after_force (shared.rs:141-148) for particle b with acceleration a: the kick, then the half
// drift with the new velocity -- k_kick_drift's arithmetic (a*dt and (v*0.5)*dt are rounded products, then added) for the
// kernels that hold a particle's finished sum and take the integration along.
template <class V4, class F>
__device__ __forceinline__ void kick_half_drift(V4* __restrict__ pos, V4* __restrict__ vel, int b, F ax, F ay, F az, F dt) {
    V4 p = pos[b], v = vel[b];
    v.x += ax * dt;                 // shared.rs:144
    v.y += ay * dt;
    v.z += az * dt;
    p.x += (v.x * Real<F>::half) * dt;     // shared.rs:146
    p.y += (v.y * Real<F>::half) * dt;
    p.z += (v.z * Real<F>::half) * dt;
    vel[b] = v;
    pos[b] = p;
}

}  // namespace nbody
