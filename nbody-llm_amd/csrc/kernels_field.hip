// kernels_field.hip -- nbody_field_at and nbody_tidal_at (NBODY_POTENTIAL_PAIRS) and the reduction both modes share; the
// quantity is a Term of probe_term.h.
//   k_probe_pairs   one-sided (a probe is not a body: nothing to credit back, so no symmetric rotation).  A lane keeps NP
//                   probes in registers, 3 coordinates + Term::kSums sums each in f64; the live bodies of every segment,
//                   concatenated in segment order, come through the wave's LDS tile (partner_stream.h).  Wave gw = group * K +
//                   slice sums slice `slice` of the body list for probes group*64*NP .. : K slices let a few thousand probes
//                   fill the chip.  Coordinates are widened to f64 as they are loaded; a body with r2 == 0 exactly gives no term.
//   k_probe_reduce  planes added in plane order, times g, to the caller's place (TREE: through the sorted index).
// Every plane row is written exactly once per batch and there are no atomics: the same bits from run to run.
#include "kernels_field.h"
#include "partner_stream.h"
#include "probe_term.h"

namespace nbody {

namespace {

// the probe as the handle sees it: rounded to the nearest f32 once on f32 handles
__device__ __forceinline__ double round_to(const float4*, double v) { return double(float(v)); }
__device__ __forceinline__ double round_to(const double4*, double v) { return v; }

template <class P, int NP, class Term>
__global__ __launch_bounds__(256) void k_probe_pairs(const P* __restrict__ pos_all, const int* __restrict__ seg_count, int n_seg, int seg_cap,
                                                     const double* __restrict__ xyz, int n, int groups, int K, double* __restrict__ planes,
                                                     size_t plane_stride, double eps2) {
    __shared__ double4 tile[4][64];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int gw = blockIdx.x * 4 + wv;
    if (gw >= groups * K) return;
    const int group = gw / K, slice = gw - group * K;
    double x[NP], y[NP], z[NP], sums[NP][Term::kSums];
#pragma unroll
    for (int q = 0; q < NP; ++q) {
        const int i = (group * NP + q) * 64 + lane;
        const bool live = i < n;
        x[q] = live ? round_to(pos_all, xyz[3 * size_t(i)]) : 0.0;
        y[q] = live ? round_to(pos_all, xyz[3 * size_t(i) + 1]) : 0.0;
        z[q] = live ? round_to(pos_all, xyz[3 * size_t(i) + 2]) : 0.0;
#pragma unroll
        for (int u = 0; u < Term::kSums; ++u) sums[q][u] = 0.0;
    }
    stream_partners(
        tile[wv], lane, pos_all, seg_cap, n_seg, [&](int sg) { return Win{sg, 0, min(max(seg_count[sg], 0), seg_cap)}; }, slice, K,
        [&](const double4 pj, int, int) {
#pragma unroll
            for (int q = 0; q < NP; ++q) {
                const double dx = pj.x - x[q], dy = pj.y - y[q], dz = pj.z - z[q];
                const double r2 = (dx * dx + dy * dy) + dz * dz;
                Term::add(sums[q], dx, dy, dz, pj.w, r2 + eps2, r2 == 0.0);   // a probe on a body: no term from that body
            }
        });
#pragma unroll
    for (int q = 0; q < NP; ++q) {
        const int i = (group * NP + q) * 64 + lane;
        if (i < n) store_probe_row(planes, slice, plane_stride, i, sums[q], isfinite(x[q]) && isfinite(y[q]) && isfinite(z[q]));
    }
}

template <class Term>
__global__ __launch_bounds__(256) void k_probe_reduce(const double* __restrict__ planes, int K, size_t plane_stride, const int* __restrict__ idx,
                                                      int n, double g, double* __restrict__ acc, double* __restrict__ phi) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    double sums[Term::kSums] = {};
    for (int k = 0; k < K; ++k) {   // plane order
        const double2* __restrict__ row = reinterpret_cast<const double2*>(planes + (size_t(k) * plane_stride + t) * Term::kSums);
#pragma unroll
        for (int u = 0; u < Term::kSums / 2; ++u) {
            const double2 v = row[u];
            sums[2 * u] += v.x; sums[2 * u + 1] += v.y;
        }
    }
    Term::write(sums, g, idx ? size_t(idx[t]) : size_t(t), acc, phi);
}

template <class Term> constexpr int probes_per_lane(size_t n) { return n <= size_t(kOnePerLaneUpTo) ? 1 : Term::kPairsNP; }

template <class P, class Term>
void pairs_impl(hipStream_t s, const PotBodies& b, const double* xyz, int n, int K, double eps2, double* planes, size_t stride) {
    const P* pos_all = static_cast<const P*>(b.pos_all);
    const int np = probes_per_lane<Term>(n), groups = (n + 64 * np - 1) / (64 * np);
    const dim3 grid((groups * K + 3) / 4), block(256);
    if (np == 1)
        hipLaunchKernelGGL((k_probe_pairs<P, 1, Term>), grid, block, 0, s, pos_all, b.seg_count, b.n_seg, b.seg_cap, xyz, n, groups, K, planes, stride, eps2);
    else
        hipLaunchKernelGGL((k_probe_pairs<P, Term::kPairsNP, Term>), grid, block, 0, s, pos_all, b.seg_count, b.n_seg, b.seg_cap, xyz, n, groups, K, planes,
                           stride, eps2);
}

template <class Term>
int slices_impl(size_t n, size_t n_bodies) {
    const size_t per = 64 * size_t(probes_per_lane<Term>(n)), groups = (n + per - 1) / per;
    size_t K = 4096 / (groups ? groups : 1);                       // ~4 waves per SIMD of 256 CUs
    K = K < (n_bodies + 255) / 256 ? K : (n_bodies + 255) / 256;   // (a slice of fewer than 256 bodies is not worth a wave)
    return int(K < 1 ? 1 : K > 64 ? 64 : K);
}

}  // namespace

int probe_pairs_slices(ProbeTerm term, size_t n, size_t n_bodies) {
    return probe_tidal(term) ? slices_impl<TidalTerm<true>>(n, n_bodies) : slices_impl<FieldTerm<true, true>>(n, n_bodies);
}

void launch_probe_pairs(hipStream_t s, ProbeTerm term, const PotBodies& b, const double* xyz, int n, int K, double eps2, double* planes, size_t stride) {
    if (n <= 0 || probe_counts_only(term)) return;
    if (probe_tidal(term)) {
        if (b.f64) pairs_impl<double4, TidalTerm<true>>(s, b, xyz, n, K, eps2, planes, stride);
        else pairs_impl<float4, TidalTerm<true>>(s, b, xyz, n, K, eps2, planes, stride);
    } else {
        if (b.f64) pairs_impl<double4, FieldTerm<true, true>>(s, b, xyz, n, K, eps2, planes, stride);
        else pairs_impl<float4, FieldTerm<true, true>>(s, b, xyz, n, K, eps2, planes, stride);
    }
}

void launch_probe_reduce(hipStream_t s, ProbeTerm term, const double* planes, int K, size_t stride, const int* idx, int n, double g, double* acc,
                         double* phi) {
    if (n <= 0 || (!acc && !phi)) return;
    const dim3 grid((n + 255) / 256), block(256);
    if (probe_tidal(term)) hipLaunchKernelGGL(k_probe_reduce<TidalTerm<true>>, grid, block, 0, s, planes, K, stride, idx, n, g, acc, phi);
    else hipLaunchKernelGGL((k_probe_reduce<FieldTerm<true, true>>), grid, block, 0, s, planes, K, stride, idx, n, g, acc, phi);
}

}  // namespace nbody
