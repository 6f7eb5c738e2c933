// kernels_external.hip -- the static external field on the device (gfx950): external_field.h's expressions, one body, tracer
// or probe per lane.  Pure streaming kernels; compiled with -ffp-contract=off (every product and sum rounded on its own).
//
//   k_ext_add  acc += s(pos) after the force pass, in the handle's precision, with the leapfrog's kick + half drift when a
//              step asks for it (k_kick_drift's operations on the acceleration just stored)
//   k_ext_phi  f64 potentials of the bodies and the block sums of m phi, added in a fixed tree: no floating-point atomics,
//              the same input gives the same bits
//   k_ext_at   f64 acceleration and potential at probes
#include "kernels_external.h"
#include "real.h"   // Real<F>, widen, kick_half_drift

#include <algorithm>

namespace nbody {

// (the kernels live in namespace nbody like every other kernel of the library: their handles are the only data symbols it exports)
using ext::FieldT;
using ext::kExtBlock;

template <class F>
__global__ __launch_bounds__(kExtBlock) void k_ext_add(typename Real<F>::V4* __restrict__ pos, typename Real<F>::V4* __restrict__ vel,
                                                       typename Real<F>::V4* __restrict__ acc, const int* __restrict__ count,
                                                       const FieldT<F> f, F g, int do_kick, F dt, int* __restrict__ poison, int count_step) {
    if (poison && *poison) return;
    const int k = blockIdx.x * kExtBlock + threadIdx.x;
    if (k == 0 && poison && count_step) atomicAdd(poison + 1, 1);   // a step of an unsynchronised Barnes-Hut run is complete
    if (k >= *count) return;
    const typename Real<F>::V4 p = pos[k];
    typename Real<F>::V4 a = acc[k];
    F s[3];
    ext::acc_sum(f, g, p.x, p.y, p.z, s);
    a.x = a.x + s[0];
    a.y = a.y + s[1];
    a.z = a.z + s[2];
    acc[k] = a;
    if (do_kick) kick_half_drift(pos, vel, k, a.x, a.y, a.z, dt);
}

template <class F>
__global__ __launch_bounds__(kExtBlock) void k_ext_phi(const typename Real<F>::V4* __restrict__ pos, const int* __restrict__ count,
                                                       const FieldT<double> f, double g, double* __restrict__ phi,
                                                       double* __restrict__ part) {
    __shared__ double sum[kExtBlock];
    const int t = threadIdx.x;
    const int k = blockIdx.x * kExtBlock + t;
    double mphi = 0.0;
    if (k < *count) {
        const double4 p = widen(pos[k]);
        const double v = ext::phi_sum(f, g, p.x, p.y, p.z);
        if (phi) phi[k] = v;
        mphi = p.w * v;
    }
    sum[t] = mphi;
    __syncthreads();
    for (int half = kExtBlock / 2; half > 0; half >>= 1) {   // sum[t] += sum[t + half]: the same pairs whatever the schedule
        if (t < half) sum[t] = sum[t] + sum[t + half];
        __syncthreads();
    }
    if (t == 0) part[blockIdx.x] = sum[0];
}

__global__ __launch_bounds__(kExtBlock) void k_ext_at(const double* __restrict__ xyz, int n, const FieldT<double> f, double g,
                                                      double* __restrict__ acc, double* __restrict__ phi) {
    const int k = blockIdx.x * kExtBlock + threadIdx.x;
    if (k >= n) return;
    const double p[3] = {xyz[3 * size_t(k)], xyz[3 * size_t(k) + 1], xyz[3 * size_t(k) + 2]};
    double a[3], v;
    ext::eval_point(f, g, p, acc ? a : nullptr, phi ? &v : nullptr);
    if (acc) { acc[3 * size_t(k)] = a[0]; acc[3 * size_t(k) + 1] = a[1]; acc[3 * size_t(k) + 2] = a[2]; }
    if (phi) phi[k] = v;
}

namespace ext {

template <class F>
void launch_ext_add(hipStream_t s, const ShardT<F>& sh, int n_upper, const FieldT<F>& f, F g, const F* kick_dt, bool count_step) {
    const int blocks = blocks_for(n_upper);
    if (blocks == 0 && !(sh.poison && count_step)) return;
    hipLaunchKernelGGL(k_ext_add<F>, dim3(std::max(1, blocks)), dim3(kExtBlock), 0, s, sh.own_pos(), sh.vel, sh.acc, sh.own_count(), f, g,
                       kick_dt ? 1 : 0, kick_dt ? *kick_dt : F(0), sh.poison, count_step ? 1 : 0);
}

template <class F>
void launch_ext_phi(hipStream_t s, const ShardT<F>& sh, int n_upper, const FieldT<double>& f, double g, double* phi, double* part) {
    const int blocks = blocks_for(n_upper);
    if (blocks == 0) return;
    hipLaunchKernelGGL(k_ext_phi<F>, dim3(blocks), dim3(kExtBlock), 0, s, sh.own_pos(), sh.own_count(), f, g, phi, part);
}

void launch_ext_at(hipStream_t s, const double* xyz, int n, const FieldT<double>& f, double g, double* acc, double* phi) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_ext_at, dim3(blocks_for(n)), dim3(kExtBlock), 0, s, xyz, n, f, g, acc, phi);
}

template void launch_ext_add<float>(hipStream_t, const ShardT<float>&, int, const FieldT<float>&, float, const float*, bool);
template void launch_ext_add<double>(hipStream_t, const ShardT<double>&, int, const FieldT<double>&, double, const double*, bool);
template void launch_ext_phi<float>(hipStream_t, const ShardT<float>&, int, const FieldT<double>&, double, double*, double*);
template void launch_ext_phi<double>(hipStream_t, const ShardT<double>&, int, const FieldT<double>&, double, double*, double*);

}}  // namespace nbody::ext
