// dd_sum.h -- the double-double sums {m, m x, m y, m z} of the device tree build (kernels_tree.hip) and of the spatial ranks'
// spanning cells (kernels_let.hip): the arithmetic stated once.  Compiled with -ffp-contract=off (the error terms below are
// what a contracted expression would throw away).
#pragma once
#include <hip/hip_runtime.h>

namespace nbody {

struct Sum4 { double m, x, y, z; };
// The prefix sums are double-double: hi + lo, |lo| <= ulp(hi) / 2, every component of {m, m x, m y, m z} its own pair.  A cell's
// sums are differences of two prefixes, and a difference carries the rounding of everything sorted before the cell: in
// plain f64 that is 2^-53 of the prefix (a two-body cell of 1e-12 dust behind a body of mass 1 lost its centre of mass
// altogether), in double-double about 2^-100 of it (the count is in tests/tree_moments.py).
struct DD4 { Sum4 hi, lo; };

// s + e = a + b exactly (Knuth; no assumption on the sizes)
__device__ __forceinline__ void two_sum(double a, double b, double& s, double& e) {
    s = a + b;
    const double bb = s - a;
    e = (a - (s - bb)) + (b - bb);
}
// the same for |a| >= |b| (Dekker)
__device__ __forceinline__ void fast_two_sum(double a, double b, double& s, double& e) {
    s = a + b;
    e = b - (s - a);
}
// (ah + al) + (bh + bl), the accurate variant: the error is a few 2^-106 of |a + b| even when the high parts cancel, which is
// what taking a difference of prefixes does
__device__ __forceinline__ void dd_add(double ah, double al, double bh, double bl, double& rh, double& rl) {
    double s, e, t, f;
    two_sum(ah, bh, s, e);
    two_sum(al, bl, t, f);
    e += t;
    fast_two_sum(s, e, s, e);
    e += f;
    fast_two_sum(s, e, rh, rl);
}
// upto - before, rounded to one double per component (hi of the normalised difference is the double nearest to it)
__device__ __forceinline__ Sum4 dd4_diff(const DD4& upto, const DD4& before) {
    Sum4 r;
    double lo;
    dd_add(upto.hi.m, upto.lo.m, -before.hi.m, -before.lo.m, r.m, lo);
    dd_add(upto.hi.x, upto.lo.x, -before.hi.x, -before.lo.x, r.x, lo);
    dd_add(upto.hi.y, upto.lo.y, -before.hi.y, -before.lo.y, r.y, lo);
    dd_add(upto.hi.z, upto.lo.z, -before.hi.z, -before.lo.z, r.z, lo);
    return r;
}

}  // namespace nbody
