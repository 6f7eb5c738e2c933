// kernels_tidal.hip -- nbody_tidal_at(NBODY_POTENTIAL_PAIRS) and the reduction both modes share (kernels_tidal.h has the term).
//   k_tidal_pairs   k_field_pairs (kernels_field.hip) with six sums per probe: one-sided, wave gw = group * K + slice sums
//                   slice `slice` of the concatenated live bodies for probes group*64*NP .., the bodies arrive 64 at a time
//                   through the wave's own LDS tile and every read from it is a wave-uniform broadcast.  A lane keeps NP
//                   probes, 3 coordinates + 6 sums each in f64; a body with r2 == 0 exactly gives no term.
//   k_tidal_reduce  planes added in plane order, times g, to the caller's row (TREE: through the sorted index).
// Every plane row is written exactly once per batch and there are no atomics: the same bits from run to run.
#include "kernels_tidal.h"
#include "real.h"   // widen

namespace nbody {

namespace {

// probes per lane: one while that leaves the chip short of waves (as k_field_pairs), kTidalNP from there.  Nine doubles of
// state per probe: the compiler reports 58 VGPRs at 1 (8 waves per SIMD), 86 at 2 (5 waves: above the ~4 the slice count aims
// at) and 144 at 4 (3 waves), no scratch at any
constexpr int kTidalNP = 2;
constexpr int kTidalOnePerLaneUpTo = 16384;

// the probe as the handle sees it: rounded to the nearest f32 once on f32 handles
__device__ __forceinline__ double round_to(const float4*, double v) { return double(float(v)); }
__device__ __forceinline__ double round_to(const double4*, double v) { return v; }

template <class P, int NP>
__global__ __launch_bounds__(256) void k_tidal_pairs(const P* __restrict__ pos_all, const int* __restrict__ seg_count, int n_seg, int seg_cap,
                                                     const double* __restrict__ xyz, int n, int groups, int K, double2* __restrict__ planes,
                                                     size_t plane_stride, double eps2) {
    __shared__ double4 tile[4][64];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int gw = blockIdx.x * 4 + wv;
    if (gw >= groups * K) return;
    const int group = gw / K, slice = gw - group * K;
    double x[NP], y[NP], z[NP], xx[NP], xy[NP], xz[NP], yy[NP], yz[NP], zz[NP];
#pragma unroll
    for (int q = 0; q < NP; ++q) {
        const int i = (group * NP + q) * 64 + lane;
        const bool live = i < n;
        x[q] = live ? round_to(pos_all, xyz[3 * size_t(i)]) : 0.0;
        y[q] = live ? round_to(pos_all, xyz[3 * size_t(i) + 1]) : 0.0;
        z[q] = live ? round_to(pos_all, xyz[3 * size_t(i) + 2]) : 0.0;
        xx[q] = xy[q] = xz[q] = yy[q] = yz[q] = zz[q] = 0.0;
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
                        const double k3 = self ? 0.0 : (3.0 * k) / qq;
                        const double ux = dx * k3, uy = dy * k3, uz = dz * k3;
                        xx[q] += dx * ux - k; yy[q] += dy * uy - k; zz[q] += dz * uz - k;
                        xy[q] += dx * uy; xz[q] += dx * uz; yz[q] += dy * uz;
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
        double2* __restrict__ row = planes + (size_t(slice) * plane_stride + i) * kTidalRow;
        row[0] = finite ? make_double2(xx[q], xy[q]) : make_double2(bad, bad);
        row[1] = finite ? make_double2(xz[q], yy[q]) : make_double2(bad, bad);
        row[2] = finite ? make_double2(yz[q], zz[q]) : make_double2(bad, bad);
    }
}

__global__ __launch_bounds__(256) void k_tidal_reduce(const double2* __restrict__ planes, int K, size_t plane_stride, const int* __restrict__ idx,
                                                      int n, double g, double* __restrict__ out) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    double2 a = make_double2(0.0, 0.0), b = a, c = a;
    for (int k = 0; k < K; ++k) {   // plane order
        const double2* __restrict__ row = planes + (size_t(k) * plane_stride + t) * kTidalRow;
        const double2 r0 = row[0], r1 = row[1], r2 = row[2];
        a.x += r0.x; a.y += r0.y; b.x += r1.x; b.y += r1.y; c.x += r2.x; c.y += r2.y;
    }
    double2* __restrict__ o = reinterpret_cast<double2*>(out + 6 * (idx ? size_t(idx[t]) : size_t(t)));   // (48-byte rows of an allocation: 16-byte aligned)
    o[0] = make_double2(g * a.x, g * a.y); o[1] = make_double2(g * b.x, g * b.y); o[2] = make_double2(g * c.x, g * c.y);
}

template <class P>
void pairs_impl(hipStream_t s, const PotBodies& b, const double* xyz, int n, int K, double eps2, double2* planes, size_t stride) {
    const P* pos_all = static_cast<const P*>(b.pos_all);
    if (n <= kTidalOnePerLaneUpTo) {
        const int groups = (n + 63) / 64;
        hipLaunchKernelGGL((k_tidal_pairs<P, 1>), dim3((groups * K + 3) / 4), dim3(256), 0, s, pos_all, b.seg_count, b.n_seg, b.seg_cap, xyz, n, groups, K,
                           planes, stride, eps2);
    } else {
        const int groups = (n + 64 * kTidalNP - 1) / (64 * kTidalNP);
        hipLaunchKernelGGL((k_tidal_pairs<P, kTidalNP>), dim3((groups * K + 3) / 4), dim3(256), 0, s, pos_all, b.seg_count, b.n_seg, b.seg_cap, xyz, n, groups,
                           K, planes, stride, eps2);
    }
}

}  // namespace

int tidal_pairs_slices(size_t n, size_t n_bodies) {
    const size_t groups = n <= size_t(kTidalOnePerLaneUpTo) ? (n + 63) / 64 : (n + 64 * kTidalNP - 1) / (64 * kTidalNP);
    size_t K = 4096 / (groups ? groups : 1);                       // ~4 waves per SIMD of 256 CUs
    K = K < (n_bodies + 255) / 256 ? K : (n_bodies + 255) / 256;   // (a slice of fewer than 256 bodies is not worth a wave)
    return int(K < 1 ? 1 : K > 64 ? 64 : K);
}

void launch_tidal_pairs(hipStream_t s, const PotBodies& b, const double* xyz, int n, int K, double eps2, double2* planes, size_t stride) {
    if (n <= 0) return;
    if (b.f64) pairs_impl<double4>(s, b, xyz, n, K, eps2, planes, stride);
    else pairs_impl<float4>(s, b, xyz, n, K, eps2, planes, stride);
}

void launch_tidal_reduce(hipStream_t s, const double2* planes, int K, size_t stride, const int* idx, int n, double g, double* out) {
    if (n <= 0 || !out) return;
    hipLaunchKernelGGL(k_tidal_reduce, dim3((n + 255) / 256), dim3(256), 0, s, planes, K, stride, idx, n, g, out);
}

}  // namespace nbody
