// probe_term.h -- what one body or tree node adds at a probe, once per quantity; device code only.  The pair kernel
// (kernels_field.hip k_probe_pairs, F = double) and the tree probe walks (kernels_bh.hip k_bh_probe_walk, F = float;
// kernels_f64.hip k_bh_probe_walk64, F = double) take their term, their row of sums and their reduce from here.
//   kSums     doubles per plane row (rows are kSums / 2 consecutive double2, 16-byte aligned)
//   kAny      false: count only -- nothing is summed and no row is written
//   kPairsNP  probes per lane of the pair kernel beyond kOnePerLaneUpTo probes
//   add       d = x_j - x, q = |d|^2 + eps2, every line one rounding in F (IEEE sqrt and divide, nothing contracted), every
//             product widened to the f64 sum it is added to.  none: the pair kernel's r2 == 0 rule, no term from that body
//   write     what the reduce leaves of a row of plane sums
#pragma once
#include "kernels_field.h"   // ProbeTerm
#include "real.h"

namespace nbody {

constexpr int kOnePerLaneUpTo = 16384;   // one probe per lane while that leaves the chip short of waves

// nbody_field_at: {sum m d / s^3, sum m / s}, s = sqrt(q).  inv = 1 / sqrt(q), st = m inv, k = st / q: the divide instead of
// two more products with inv keeps a component within 15 u of its exact value (tests/field_list.py counts)
template <bool VEC, bool SCAL>
struct FieldTerm {
    static constexpr int kSums = 4;   // {ax, ay, az, scalar}
    static constexpr bool kAny = VEC || SCAL;
    static constexpr int kPairsNP = 4;
    template <class F>
    static __device__ __forceinline__ void add(double (&s)[kSums], F dx, F dy, F dz, F m, F q, bool none) {
        const F st = m * (F(1) / Real<F>::sqrt(q));
        if (SCAL) s[3] += none ? 0.0 : double(st);
        if (VEC) {
            const F k = none ? F(0) : st / q;
            s[0] += double(dx * k); s[1] += double(dy * k); s[2] += double(dz * k);
        }
    }
    // acc [3] = +g sum, phi = -g sum; either may be null
    static __device__ __forceinline__ void write(const double (&s)[kSums], double g, size_t i, double* __restrict__ acc, double* __restrict__ phi) {
        if (acc) { acc[3 * i] = g * s[0]; acc[3 * i + 1] = g * s[1]; acc[3 * i + 2] = g * s[2]; }
        if (phi) phi[i] = -(g * s[3]);
    }
};

// nbody_tidal_at: T_ab = sum m (3 d_a d_b / q^(5/2) - delta_ab / q^(3/2)) as {xx, xy, xz, yy, yz, zz}.
//     inv = 1 / sqrt(q)   st = m inv   k = st / q   k3 = (3 k) / q   u_c = d_c k3
// (the two divides by q, not products with inv, keep a component within 24 u of the term's scale: tests/tidal_list.py counts).
// In f32 the accepted nodes are 1e-5 away or more, so k3 <= 3 m 1e25 stays in range; with r2 = inf: inv = k = k3 = 0 and finite
// d times 0: exact zeros.
// Probes per lane of the pair kernel: nine doubles of state per probe; the compiler reports 58 VGPRs at 1 (8 waves per SIMD),
// 86 at 2 (5 waves: above the ~4 the slice count aims at) and 144 at 4 (3 waves), no scratch at any
template <bool SUMS>
struct TidalTerm {
    static constexpr int kSums = 6;
    static constexpr bool kAny = SUMS;
    static constexpr int kPairsNP = 2;
    template <class F>
    static __device__ __forceinline__ void add(double (&s)[kSums], F dx, F dy, F dz, F m, F q, bool none) {
        const F st = m * (F(1) / Real<F>::sqrt(q));
        const F k = none ? F(0) : st / q;
        const F k3 = none ? F(0) : (F(3) * k) / q;
        const F ux = dx * k3, uy = dy * k3, uz = dz * k3;
        s[0] += double(dx * ux - k); s[3] += double(dy * uy - k); s[5] += double(dz * uz - k);
        s[1] += double(dx * uy); s[2] += double(dx * uz); s[4] += double(dy * uz);
    }
    // out [6] = g sum (48-byte rows of an allocation: 16-byte aligned)
    static __device__ __forceinline__ void write(const double (&s)[kSums], double g, size_t i, double* __restrict__ out, double*) {
        double2* __restrict__ o = reinterpret_cast<double2*>(out + 6 * i);
        o[0] = make_double2(g * s[0], g * s[1]); o[1] = make_double2(g * s[2], g * s[3]); o[2] = make_double2(g * s[4], g * s[5]);
    }
};

// a probe's row of plane `plane`: the sums, or NaN for a non-finite probe
template <int SUMS>
__device__ __forceinline__ void store_probe_row(double* __restrict__ planes, size_t plane, size_t plane_stride, size_t t, const double (&s)[SUMS], bool finite) {
    const double bad = __longlong_as_double(0x7ff8000000000000ll);
    double2* __restrict__ row = reinterpret_cast<double2*>(planes + (plane * plane_stride + t) * SUMS);
#pragma unroll
    for (int u = 0; u < SUMS / 2; ++u) row[u] = finite ? make_double2(s[2 * u], s[2 * u + 1]) : make_double2(bad, bad);
}

// host side: the Term of a call (kernels_field.h ProbeTerm), as a template argument
#define NBODY_PROBE_TERM(term, CALL)                                           \
    switch (term) {                                                            \
        case nbody::ProbeTerm::Field: { using Term = nbody::FieldTerm<true, true>; CALL; break; }       \
        case nbody::ProbeTerm::FieldAcc: { using Term = nbody::FieldTerm<true, false>; CALL; break; }   \
        case nbody::ProbeTerm::FieldPhi: { using Term = nbody::FieldTerm<false, true>; CALL; break; }   \
        case nbody::ProbeTerm::FieldCount: { using Term = nbody::FieldTerm<false, false>; CALL; break; } \
        case nbody::ProbeTerm::Tidal: { using Term = nbody::TidalTerm<true>; CALL; break; }             \
        case nbody::ProbeTerm::TidalCount: { using Term = nbody::TidalTerm<false>; CALL; break; }       \
    }

}  // namespace nbody
