// kernels_field.hip -- nbody_field_at(NBODY_POTENTIAL_PAIRS) and the reduction both modes share.
//   k_field_pairs   one-sided (a probe is not a body: nothing to credit back, so no symmetric rotation).  A lane keeps NP
//                   probes in registers, 3 coordinates + 4 sums each in f64; the live bodies of every segment, concatenated in
//                   segment order, arrive 64 at a time through the wave's LDS tile (kernels_pot.hip k_pot_os) and every body read
//                   from it is a wave-uniform broadcast.  Wave gw = group * K + slice sums slice `slice` of the body list for
//                   probes group*64*NP .. : K slices let a few thousand probes fill the chip.  Coordinates are widened to f64
//                   as they are loaded; a term is q = r2 + eps2, inv = 1 / sqrt(q) (IEEE sqrt and divide), scalar m * inv,
//                   vector d * ((m * inv) / q); a body with r2 == 0 exactly is skipped.
//   k_field_reduce  planes added in plane order, times +g / -g, to the caller's place (TREE: through the sorted index).
// Every plane entry is written exactly once per batch and there are no atomics: the same bits from run to run.
#include "kernels_field.h"
#include "real.h"   // widen

namespace nbody {

namespace {

// the probe as the handle sees it: rounded to the nearest f32 once on f32 handles
__device__ __forceinline__ double round_to(const float4*, double v) { return double(float(v)); }
__device__ __forceinline__ double round_to(const double4*, double v) { return v; }

template <class P, int NP>
__global__ __launch_bounds__(256) void k_field_pairs(const P* __restrict__ pos_all, const int* __restrict__ seg_count, int n_seg, int seg_cap,
                                                     const double* __restrict__ xyz, int n, int groups, int K, double4* __restrict__ planes,
                                                     size_t plane_stride, double eps2) {
    __shared__ double4 tile[4][64];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int gw = blockIdx.x * 4 + wv;
    if (gw >= groups * K) return;
    const int group = gw / K, slice = gw - group * K;
    double x[NP], y[NP], z[NP], ax[NP], ay[NP], az[NP], sm[NP];
#pragma unroll
    for (int q = 0; q < NP; ++q) {
        const int i = (group * NP + q) * 64 + lane;
        const bool live = i < n;
        x[q] = live ? round_to(pos_all, xyz[3 * size_t(i)]) : 0.0;
        y[q] = live ? round_to(pos_all, xyz[3 * size_t(i) + 1]) : 0.0;
        z[q] = live ? round_to(pos_all, xyz[3 * size_t(i) + 2]) : 0.0;
        ax[q] = ay[q] = az[q] = sm[q] = 0.0;
    }
    long long R = 0;
    for (int sg = 0; sg < n_seg; ++sg) R += min(max(seg_count[sg], 0), seg_cap);
    const long long r0 = R * slice / K, r1 = R * (slice + 1) / K;
    long long first = 0;   // index of the segment's first body in the concatenated list
    for (int sg = 0; sg < n_seg; ++sg) {
        const int len = min(max(seg_count[sg], 0), seg_cap);
        const long long lo = max(r0, first), hi = min(r1, first + len);
        if (lo < hi) {
            const P* __restrict__ ps = pos_all + size_t(sg) * seg_cap;   // ps[c - first]: body c of the list
            const double4 none = make_double4(0.0, 0.0, 0.0, 0.0);
            double4 nxt = (lo + lane < hi) ? widen(ps[lo + lane - first]) : none;
            for (long long c0 = lo; c0 < hi; c0 += 64) {
                tile[wv][lane] = nxt;   // the wave's own tile: its LDS operations complete in program order
                if (c0 + 64 + lane < hi) nxt = widen(ps[c0 + 64 + lane - first]);
                const int cnt = int(min(64LL, hi - c0));
                for (int t = 0; t < cnt; ++t) {
                    const double4 pj = tile[wv][t];   // wave-uniform address: an LDS broadcast
#pragma unroll
                    for (int q = 0; q < NP; ++q) {
                        const double dx = pj.x - x[q], dy = pj.y - y[q], dz = pj.z - z[q];
                        const double r2 = (dx * dx + dy * dy) + dz * dz;
                        const double qq = r2 + eps2;
                        const double st = pj.w * (1.0 / __builtin_sqrt(qq));
                        const bool self = r2 == 0.0;   // a probe on a body: no term from that body
                        const double k = self ? 0.0 : st / qq;
                        sm[q] += self ? 0.0 : st;
                        ax[q] += dx * k; ay[q] += dy * k; az[q] += dz * k;
                    }
                }
            }
        }
        first += len;
    }
#pragma unroll
    for (int q = 0; q < NP; ++q) {
        const int i = (group * NP + q) * 64 + lane;
        if (i >= n) continue;
        const bool finite = isfinite(x[q]) && isfinite(y[q]) && isfinite(z[q]);
        const double bad = __longlong_as_double(0x7ff8000000000000ll);
        planes[size_t(slice) * plane_stride + i] = finite ? make_double4(ax[q], ay[q], az[q], sm[q]) : make_double4(bad, bad, bad, bad);
    }
}

__global__ __launch_bounds__(256) void k_field_reduce(const double4* __restrict__ planes, int K, size_t plane_stride, const int* __restrict__ idx,
                                                      int n, double g, double* __restrict__ acc, double* __restrict__ phi) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    double sx = 0.0, sy = 0.0, sz = 0.0, sw = 0.0;
    for (int k = 0; k < K; ++k) {   // plane order
        const double4 v = planes[size_t(k) * plane_stride + t];
        sx += v.x; sy += v.y; sz += v.z; sw += v.w;
    }
    const size_t i = idx ? size_t(idx[t]) : size_t(t);
    if (acc) { acc[3 * i] = g * sx; acc[3 * i + 1] = g * sy; acc[3 * i + 2] = g * sz; }
    if (phi) phi[i] = -(g * sw);
}

template <class P>
void pairs_impl(hipStream_t s, const PotBodies& b, const double* xyz, int n, int K, double eps2, double4* planes, size_t stride) {
    const P* pos_all = static_cast<const P*>(b.pos_all);
    // one probe per lane while that leaves the chip short of waves, four from there
    if (n <= 16384) {
        const int groups = (n + 63) / 64;
        hipLaunchKernelGGL((k_field_pairs<P, 1>), dim3((groups * K + 3) / 4), dim3(256), 0, s, pos_all, b.seg_count, b.n_seg, b.seg_cap, xyz, n, groups, K,
                           planes, stride, eps2);
    } else {
        const int groups = (n + 255) / 256;
        hipLaunchKernelGGL((k_field_pairs<P, 4>), dim3((groups * K + 3) / 4), dim3(256), 0, s, pos_all, b.seg_count, b.n_seg, b.seg_cap, xyz, n, groups, K,
                           planes, stride, eps2);
    }
}

}  // namespace

int field_pairs_slices(size_t n, size_t n_bodies) {
    const size_t groups = n <= 16384 ? (n + 63) / 64 : (n + 255) / 256;
    size_t K = 4096 / (groups ? groups : 1);                       // ~4 waves per SIMD of 256 CUs
    K = K < (n_bodies + 255) / 256 ? K : (n_bodies + 255) / 256;   // (a slice of fewer than 256 bodies is not worth a wave)
    return int(K < 1 ? 1 : K > 64 ? 64 : K);
}

void launch_field_pairs(hipStream_t s, const PotBodies& b, const double* xyz, int n, int K, double eps2, double4* planes, size_t stride) {
    if (n <= 0) return;
    if (b.f64) pairs_impl<double4>(s, b, xyz, n, K, eps2, planes, stride);
    else pairs_impl<float4>(s, b, xyz, n, K, eps2, planes, stride);
}

void launch_field_reduce(hipStream_t s, const double4* planes, int K, size_t stride, const int* idx, int n, double g, double* acc, double* phi) {
    if (n <= 0 || (!acc && !phi)) return;
    hipLaunchKernelGGL(k_field_reduce, dim3((n + 255) / 256), dim3(256), 0, s, planes, K, stride, idx, n, g, acc, phi);
}

}  // namespace nbody
