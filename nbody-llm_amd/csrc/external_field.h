// external_field.h -- the static external field's per-kind expressions (include/nbody_hip.h, "external field"), stated once:
// the kernels (kernels_external.hip) and nbody_host_external_eval (nbody_external.cpp) both evaluate these functions.
//
// Every translation unit that includes this header is compiled with -ffp-contract=off: every product and sum below is
// rounded on its own, sqrt and divide are IEEE, and the order of operations is the one the public header fixes -- so
// F = float on the device, F = double on the device and F = double on the host give the bits of the numpy restatement
// (tests/external_ref.py).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/nbody_hip.h"

namespace nbody { namespace ext {

// one component in the precision F of the pass (centre and parameters rounded to F once); 64 bytes for F = double
template <class F>
struct CompT {
    int kind;
    int reserved;
    F c[3];
    F p[4];
};
// the field as a kernel argument, by value: at most NBODY_EXTERNAL_MAX components
template <class F>
struct FieldT {
    int n;
    int reserved;
    CompT<F> c[NBODY_EXTERNAL_MAX];
};

__host__ __device__ inline float sqrt_ieee(float x) { return __builtin_sqrtf(x); }
__host__ __device__ inline double sqrt_ieee(double x) { return __builtin_sqrt(x); }

// term = the component's acceleration at (x, y, z); exact zeros where the header says the term is skipped
template <class F>
__host__ __device__ inline void acc_term(const CompT<F>& k, F g, F x, F y, F z, F t[3]) {
    const F dx = x - k.c[0], dy = y - k.c[1], dz = z - k.c[2];
    t[0] = t[1] = t[2] = F(0);
    switch (k.kind) {
        case NBODY_EXT_PLUMMER: {   // p = {M, b}
            const F r2 = ((dx * dx + dy * dy) + dz * dz) + k.p[1] * k.p[1];
            if (r2 == F(0)) return;
            const F r = sqrt_ieee(r2);
            const F f = (g * k.p[0]) / (r2 * r);
            t[0] = -(dx * f); t[1] = -(dy * f); t[2] = -(dz * f);
            return;
        }
        case NBODY_EXT_HERNQUIST: {   // p = {M, a}
            const F r = sqrt_ieee((dx * dx + dy * dy) + dz * dz);
            if (r == F(0)) return;
            const F ra = r + k.p[1];
            const F f = (g * k.p[0]) / (r * (ra * ra));
            t[0] = -(dx * f); t[1] = -(dy * f); t[2] = -(dz * f);
            return;
        }
        case NBODY_EXT_MIYAMOTO_NAGAI: {   // p = {M, a, b}
            const F B = sqrt_ieee(dz * dz + k.p[2] * k.p[2]);
            const F aB = k.p[1] + B;
            const F D = (dx * dx + dy * dy) + aB * aB;
            const F f = (g * k.p[0]) / (D * sqrt_ieee(D));
            const F fz = (f * aB) / B;
            t[0] = -(dx * f); t[1] = -(dy * f); t[2] = -(dz * fz);
            return;
        }
        case NBODY_EXT_LOGARITHMIC: {   // p = {v0, rc, qy, qz}
            const F yq = dy / k.p[2], zq = dz / k.p[3];
            const F S = ((k.p[1] * k.p[1] + dx * dx) + yq * yq) + zq * zq;
            const F f = (k.p[0] * k.p[0]) / S;
            t[0] = -(dx * f);
            t[1] = -((dy / (k.p[2] * k.p[2])) * f);
            t[2] = -((dz / (k.p[3] * k.p[3])) * f);
            return;
        }
    }
}

// s = 0, then s_c += term_c for the components in ascending order
template <class F>
__host__ __device__ inline void acc_sum(const FieldT<F>& f, F g, F x, F y, F z, F s[3]) {
    s[0] = s[1] = s[2] = F(0);
    for (int k = 0; k < f.n; ++k) {
        F t[3];
        acc_term(f.c[k], g, x, y, z, t);
        s[0] += t[0]; s[1] += t[1]; s[2] += t[2];
    }
}

// the potentials: f64 whatever the handle's precision
__host__ __device__ inline double phi_term(const CompT<double>& k, double g, double x, double y, double z) {
    const double dx = x - k.c[0], dy = y - k.c[1], dz = z - k.c[2];
    switch (k.kind) {
        case NBODY_EXT_PLUMMER: {
            const double r2 = ((dx * dx + dy * dy) + dz * dz) + k.p[1] * k.p[1];
            if (r2 == 0.0) return 0.0;
            return -((g * k.p[0]) / sqrt_ieee(r2));
        }
        case NBODY_EXT_HERNQUIST: {
            const double r = sqrt_ieee((dx * dx + dy * dy) + dz * dz);
            return -((g * k.p[0]) / (r + k.p[1]));
        }
        case NBODY_EXT_MIYAMOTO_NAGAI: {
            const double B = sqrt_ieee(dz * dz + k.p[2] * k.p[2]);
            const double aB = k.p[1] + B;
            return -((g * k.p[0]) / sqrt_ieee((dx * dx + dy * dy) + aB * aB));
        }
        case NBODY_EXT_LOGARITHMIC: {
            const double yq = dy / k.p[2], zq = dz / k.p[3];
            const double S = ((k.p[1] * k.p[1] + dx * dx) + yq * yq) + zq * zq;
            return (0.5 * (k.p[0] * k.p[0])) * log(S);
        }
    }
    return 0.0;
}

__host__ __device__ inline double phi_sum(const FieldT<double>& f, double g, double x, double y, double z) {
    double s = 0.0;
    for (int k = 0; k < f.n; ++k) s += phi_term(f.c[k], g, x, y, z);
    return s;
}

// one probe of nbody_external_at / nbody_host_external_eval: acc3 and phi may be null; a probe with a non-finite coordinate
// gets NaN in everything asked for
__host__ __device__ inline void eval_point(const FieldT<double>& f, double g, const double* xyz, double* acc3, double* phi) {
    const double x = xyz[0], y = xyz[1], z = xyz[2];
    const double span = (x - x) + (y - y) + (z - z);   // 0 for finite coordinates, NaN otherwise
    if (span != 0.0) {
        if (acc3) acc3[0] = acc3[1] = acc3[2] = span;
        if (phi) *phi = span;
        return;
    }
    if (acc3) acc_sum(f, g, x, y, z, acc3);
    if (phi) *phi = phi_sum(f, g, x, y, z);
}

}}  // namespace nbody::ext
