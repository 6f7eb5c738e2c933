// kernels_tracer.hip -- the tracers' force passes for gfx950: M massless particles in the field of N bodies, one-sided.
//
//   strict : k_bf_strict's expression without a self index -- one tracer per lane, the bodies in ascending order through an
//            LDS tile, d = sqrt((x*x + y*y) + z*z + eps^2), f = g / ((d*d)*d), a -= (r*f)*m, no contraction, IEEE sqrt and
//            divide: the bits a zero-mass body appended after the bodies gets from the reference's loop.
//   fast   : k_bf_fast's pair arithmetic (FMA chain into r2, v_rsq_f32, (m*rinv)*(rinv*rinv), FMAs into the sums).  A lane
//            keeps IPT tracers in registers; a workgroup streams ONE slice of the bodies through an LDS tile that every lane
//            reads at the same (wave-uniform) address: one ds_read_b128 per 64*IPT pair evaluations.  The grid is
//            (groups of 256*IPT tracers) x (K slices).  K == 1: the sums are complete, the kernel scales them by g, stores
//            them and takes the kick + half drift along.  K > 1: every workgroup writes its rows of plane [slice] exactly
//            once, and k_tr_reduce adds the planes in plane order (and takes the kick along).  No atomics on the sums: the
//            same input gives the same bits, and a tracer's result depends on its position and the plan only.
#include "kernels_tracer.h"
#include "real.h"   // kick_half_drift

#include <algorithm>

namespace nbody {

TracerPlan tracer_plan(size_t n_tracers, size_t n_bodies) {
    TracerPlan p;
    const size_t m = std::max<size_t>(1, n_tracers), n = std::max<size_t>(1, n_bodies);
    // tracers per lane: more of them per LDS read once there are enough tracers to fill the chip anyway (256 CUs x 4
    // workgroups of 256 lanes = 262 144 lanes)
    p.ipt = m >= (size_t(1) << 19) ? 4 : m >= (size_t(1) << 17) ? 2 : 1;
    const size_t group = size_t(kTrBlock) * size_t(p.ipt);
    p.groups = int((m + group - 1) / group);
    // slices: as many as bring the launch to ~1024 workgroups, none shorter than 256 bodies, at most kTrMaxSlices
    const size_t want = (1024 + size_t(p.groups) - 1) / size_t(p.groups);
    size_t K = std::min<size_t>(std::min<size_t>(want, (n + 255) / 256), size_t(kTrMaxSlices));
    K = std::max<size_t>(K, 1);
    size_t len = (n + K - 1) / K;
    len = (len + 63) / 64 * 64;          // whole 64-body rows, so that no slice is empty:
    p.slice_len = int(len);
    p.K = int((n + len - 1) / len);      // K slices tile [0, n), the last one possibly shorter
    return p;
}

// ------------------------------------------------------------------------------------ strict
constexpr int kTrStrictBlock = 256;
constexpr int kTrStrictTile = 1024;

__global__ __launch_bounds__(kTrStrictBlock) void k_tr_bf_strict(const float4* __restrict__ body_pos, const int* __restrict__ body_count,
                                                                 const float4* __restrict__ tr_pos, const int* __restrict__ tr_count,
                                                                 float4* __restrict__ tr_acc, float g, float eps2,
                                                                 unsigned long long* __restrict__ stats) {
    __shared__ float4 tile[kTrStrictTile];
    const int tid = threadIdx.x;
    const int i = blockIdx.x * kTrStrictBlock + tid;
    const int n = *body_count, m = *tr_count;
    if (stats && blockIdx.x == 0 && tid == 0) atomicAdd(stats, (unsigned long long)m * (unsigned long long)n);
    const float4 pi = (i < m) ? tr_pos[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    float ax = 0.f, ay = 0.f, az = 0.f;
    for (int t0 = 0; t0 < n; t0 += kTrStrictTile) {
        const int cnt = min(kTrStrictTile, n - t0);
        __syncthreads();
        for (int k = tid; k < cnt; k += kTrStrictBlock) tile[k] = body_pos[t0 + k];
        __syncthreads();
        for (int j = 0; j < cnt; ++j) {
            const float4 pj = tile[j];
            const float rx = pi.x - pj.x, ry = pi.y - pj.y, rz = pi.z - pj.z;
            const float r_dist = __builtin_sqrtf((rx * rx + ry * ry) + rz * rz + eps2);
            const float r_cubed = r_dist * r_dist * r_dist;
            const float force = (g / r_cubed);
            ax -= (rx * force) * pj.w;
            ay -= (ry * force) * pj.w;
            az -= (rz * force) * pj.w;
        }
    }
    if (i < m) tr_acc[i] = make_float4(ax, ay, az, 0.f);
}

// -------------------------------------------------------------------------------------- fast
template <int IPT>
__global__ __launch_bounds__(kTrBlock) void k_tr_bf_fast(const float4* __restrict__ body_pos, const int* __restrict__ body_count,
                                                         float4* __restrict__ tr_pos, float4* __restrict__ tr_vel,
                                                         float4* __restrict__ tr_acc, const int* __restrict__ tr_count, int slice_len,
                                                         int K, float4* __restrict__ planes, size_t m_pad, float g, float eps2,
                                                         int do_kick, float dt, unsigned long long* __restrict__ stats) {
    __shared__ float4 tile[kTrTile];
    const int tid = threadIdx.x;
    const int slice = blockIdx.y;
    const int n = *body_count, m = *tr_count;
    if (stats && blockIdx.x == 0 && slice == 0 && tid == 0) atomicAdd(stats, (unsigned long long)m * (unsigned long long)n);
    const int base = blockIdx.x * (kTrBlock * IPT);

    float px[IPT], py[IPT], pz[IPT], ax[IPT], ay[IPT], az[IPT];
#pragma unroll
    for (int q = 0; q < IPT; ++q) {
        const int i = base + q * kTrBlock + tid;
        const float4 p = (i < m) ? tr_pos[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        px[q] = p.x; py[q] = p.y; pz[q] = p.z;
        ax[q] = ay[q] = az[q] = 0.f;
    }

    // the slice's bodies, from the LIVE count (a slice beyond it is empty and contributes zeros)
    const long long s0l = (long long)slice * slice_len;
    const int s0 = int(s0l < n ? s0l : n);
    const int s1 = min(n, s0 + slice_len);
    for (int t0 = s0; t0 < s1; t0 += kTrTile) {
        const int cnt = min(kTrTile, s1 - t0);
        __syncthreads();
        for (int k = tid; k < cnt; k += kTrBlock) tile[k] = body_pos[t0 + k];
        __syncthreads();
#pragma unroll 4
        for (int j = 0; j < cnt; ++j) {
            const float4 pj = tile[j];
#pragma unroll
            for (int q = 0; q < IPT; ++q) {
                const float dx = pj.x - px[q], dy = pj.y - py[q], dz = pj.z - pz[q];
                const float r2 = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, __builtin_fmaf(dx, dx, eps2)));
                const float rinv = __builtin_amdgcn_rsqf(r2);
                const float sc = (pj.w * rinv) * (rinv * rinv);
                ax[q] = __builtin_fmaf(dx, sc, ax[q]);
                ay[q] = __builtin_fmaf(dy, sc, ay[q]);
                az[q] = __builtin_fmaf(dz, sc, az[q]);
            }
        }
    }

#pragma unroll
    for (int q = 0; q < IPT; ++q) {
        const int i = base + q * kTrBlock + tid;   // < m_pad by the grid's size
        if (K > 1) {
            planes[size_t(slice) * m_pad + size_t(i)] = make_float4(ax[q], ay[q], az[q], 0.f);
        } else if (i < m) {
            const float fx = g * ax[q], fy = g * ay[q], fz = g * az[q];
            tr_acc[i] = make_float4(fx, fy, fz, 0.f);
            if (do_kick) kick_half_drift(tr_pos, tr_vel, i, fx, fy, fz, dt);
        }
    }
}

// planes [K][m_pad] -> acc, slices in ascending order, then the kick + half drift if the step asked for it
__global__ __launch_bounds__(256) void k_tr_reduce(const float4* __restrict__ planes, size_t m_pad, int K, float4* __restrict__ tr_pos,
                                                   float4* __restrict__ tr_vel, float4* __restrict__ tr_acc, const int* __restrict__ tr_count,
                                                   float g, int do_kick, float dt) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= *tr_count) return;
    float sx = 0.f, sy = 0.f, sz = 0.f;
    for (int k = 0; k < K; ++k) {
        const float4 v = planes[size_t(k) * m_pad + size_t(i)];
        sx += v.x; sy += v.y; sz += v.z;
    }
    const float fx = g * sx, fy = g * sy, fz = g * sz;
    tr_acc[i] = make_float4(fx, fy, fz, 0.f);
    if (do_kick) kick_half_drift(tr_pos, tr_vel, i, fx, fy, fz, dt);
}

void launch_tr_bf_strict(hipStream_t s, const Shard& tr, int m_upper, const Shard& bodies, float g, float g_soft2,
                         unsigned long long* stats) {
    if (m_upper <= 0) return;
    const int blocks = (m_upper + kTrStrictBlock - 1) / kTrStrictBlock;
    hipLaunchKernelGGL(k_tr_bf_strict, dim3(blocks), dim3(kTrStrictBlock), 0, s, bodies.own_pos(), bodies.own_count(), tr.own_pos(),
                       tr.own_count(), tr.acc, g, g_soft2, stats);
}

template <int IPT>
static void launch_tr_fast_cfg(hipStream_t s, const Shard& tr, const Shard& bodies, const TracerPlan& p, float4* planes, float g,
                               float eps2, const float* kick_dt, unsigned long long* stats) {
    hipLaunchKernelGGL((k_tr_bf_fast<IPT>), dim3(p.groups, p.K), dim3(kTrBlock), 0, s, bodies.own_pos(), bodies.own_count(), tr.own_pos(),
                       tr.vel, tr.acc, tr.own_count(), p.slice_len, p.K, planes, tracer_plan_pad(p), g, eps2, kick_dt ? 1 : 0,
                       kick_dt ? *kick_dt : 0.f, stats);
}

void launch_tr_bf_fast(hipStream_t s, const Shard& tr, int m_upper, const Shard& bodies, const TracerPlan& p, float4* planes,
                       float g, float g_soft2, const float* kick_dt, unsigned long long* stats) {
    if (m_upper <= 0) return;
    switch (p.ipt) {
        case 4: launch_tr_fast_cfg<4>(s, tr, bodies, p, planes, g, g_soft2, kick_dt, stats); break;
        case 2: launch_tr_fast_cfg<2>(s, tr, bodies, p, planes, g, g_soft2, kick_dt, stats); break;
        default: launch_tr_fast_cfg<1>(s, tr, bodies, p, planes, g, g_soft2, kick_dt, stats); break;
    }
    if (p.K > 1) {
        const int blocks = (m_upper + 255) / 256;
        hipLaunchKernelGGL(k_tr_reduce, dim3(blocks), dim3(256), 0, s, planes, tracer_plan_pad(p), p.K, tr.own_pos(), tr.vel, tr.acc,
                           tr.own_count(), g, kick_dt ? 1 : 0, kick_dt ? *kick_dt : 0.f);
    }
}

}  // namespace nbody
