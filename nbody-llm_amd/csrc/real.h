// real.h -- what the kernels written once for F = f32 and F = f64 need to know about the real type (the reference's
// trait is generic over Float, shared.rs:12-44): K0, K1, K3, K4 (kernels_integrate.hip) and K2 strict (kernels_bf.hip).
#pragma once
#include "kernels.h"
#include "kernels_f64.h"

namespace nbody {

template <class F> struct Real;
template <> struct Real<float> {
    using V4 = float4;
    using Bounds = BoundsF;
    static constexpr float half = 0.5f;
    static __device__ __forceinline__ V4 make4(float x, float y, float z, float w) { return make_float4(x, y, z, w); }
    static __device__ __forceinline__ float sqrt(float x) { return __builtin_sqrtf(x); }   // IEEE (-fhip-fp32-correctly-rounded-divide-sqrt)
};
template <> struct Real<double> {
    using V4 = double4;
    using Bounds = nbody64::Bounds64;
    static constexpr double half = 0.5;
    static __device__ __forceinline__ V4 make4(double x, double y, double z, double w) { return make_double4(x, y, z, w); }
    static __device__ __forceinline__ double sqrt(double x) { return __builtin_sqrt(x); }  // correctly rounded on gfx950
};

}  // namespace nbody
