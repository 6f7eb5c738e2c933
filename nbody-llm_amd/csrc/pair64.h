// pair64.h -- what the fast (NBODY_MATH_FAST) f64 all-pairs passes of kernels_bf64.hip (gravity) and kernels_hermite.hip
// (gravity and jerk) share; device code only: the padding body, the crossbar rotation and the fixed-order plane sum.
#pragma once
#include <hip/hip_runtime.h>

namespace nbody64 {
namespace pair64 {

constexpr double kPad = 1.0e100;   // zero-mass padding bodies sit far away and at rest: they exert nothing on real bodies

__device__ __forceinline__ double4 pad_body() { return make_double4(kPad, kPad, kPad, 0.0); }
__device__ __forceinline__ double4 zero4() { return make_double4(0.0, 0.0, 0.0, 0.0); }

// a double through the LDS crossbar: lane l receives lane (src_x4 / 4)'s value, two 32-bit halves
__device__ __forceinline__ double rot64(double v, int src_x4) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_ds_bpermute(src_x4, int(b));
    const int hi = __builtin_amdgcn_ds_bpermute(src_x4, int(b >> 32));
    return __longlong_as_double((long long)(unsigned)lo | ((long long)hi << 32));
}

// The fixed-order plane sum (bit-reproducible): row `row` of n_planes planes of double4[plane_stride], added in plane order,
// times g, into a; KINDS == 2: the same of a second kind of planes, kind_off entries after the first, into j.
template <int KINDS>
__device__ __forceinline__ void plane_sum(const double4* planes, int n_planes, size_t plane_stride, size_t kind_off, int row, double g, double4& a,
                                          double4& j) {
    double sx = 0.0, sy = 0.0, sz = 0.0, tx = 0.0, ty = 0.0, tz = 0.0;
    for (int p = 0; p < n_planes; ++p) {
        const double4 va = planes[size_t(p) * plane_stride + row];
        if constexpr (KINDS == 2) {
            const double4 vj = planes[kind_off + size_t(p) * plane_stride + row];
            sx += va.x; sy += va.y; sz += va.z;
            tx += vj.x; ty += vj.y; tz += vj.z;
        } else {
            sx += va.x; sy += va.y; sz += va.z;
        }
    }
    a = make_double4(g * sx, g * sy, g * sz, 0.0);
    if constexpr (KINDS == 2) j = make_double4(g * tx, g * ty, g * tz, 0.0);
}

}  // namespace pair64
}  // namespace nbody64
