// kernels_hermite.hip -- the fourth-order Hermite predictor-corrector (Makino & Aarseth 1992) of brute-force NBODY_F64
// handles: per pair the acceleration AND its time derivative, the jerk, off one shared 1/sqrt.  With d = x_j - x_i,
// w = v_j - v_i, q = |d|^2 + g_soft^2:
//     a_i = g sum_j m_j d / q^(3/2)          j_i = g sum_j m_j [ w - 3 (d.w)/q d ] / q^(3/2)
//
//   k_hm_strict     NBODY_MATH_STRICT: one body per lane, partners in ascending index order, IEEE sqrt and divide, separate
//                   multiplies and adds in the order include/nbody_hip.h states (tests/hermite_ref.py restates it bit for bit)
//   k_hm_sym        NBODY_MATH_FAST: kernels_bf64.hip's k_bf64_sym with velocities.  A wave keeps a RESIDENT SET of 64*IPT
//                   bodies in registers (position, mass, velocity, six accumulators: 13 doubles a body); TRAVELLING CHUNKS of
//                   64 bodies pass through the lanes one lane per step.  ROT = 0: the chunk's positions and velocities sit in
//                   the wave's own LDS tile, the six travelling accumulators go through the crossbar (12 ds_bpermute_b32 a
//                   step); ROT = 1: positions and velocities travel too (26 a step).
//   k_hm_os         one-sided, one body per lane, partners staged 64 at a time in the wave's LDS tile.  MODE 0: every own
//                   body (small worlds); MODE 1: the pairs k_hm_sym leaves over (the own set and, for even A, the opposite one)
//   k_hm_reduce     the planes added in a fixed order, times g; CORRECT: the corrector and the retain's flags ride along
//   k_hm_predict, k_hm_correct, k_hm_compact, k_hm_min_ratio   the small kernels of the step and of nbody_suggest_dt (the
//                   retain's look-back scan is retain.h's, shared with the leapfrog handles' k_compact)
//   k_hmb_*, k_hm_act, k_hm_act_strict   block individual time steps (nbody_set_block_steps): the schedule of a block step, F
//                   of the due bodies alone against everybody, and the corrector with the step criterion (further down)
//
// Fast pair arithmetic: rinv = rsqrt(q), rinv^2, rinv^3, nal = (-3 rinv^2) (d.w), u = w + nal d (the vector both sides
// share), one mass product per side, twelve explicit FMAs (the library builds with -ffp-contract=off).  Every plane entry
// is written exactly once per launch; there are no atomics on the planes: the same input gives the same bits.
#include "kernels_hermite.h"
#include "kernels.h"   // nbody::tuning()
#include "pair64.h"
#include "retain.h"

#include <algorithm>

namespace nbody64 {

namespace {

using namespace pair64;   // pad_body, zero4, rot64, plane_sum

// ------------------------------------------------------------------------------------------ the small kernels
// body k predicted over dt: xp = ((x0 + v0 * dt) + a0 * c2) + j0 * c3,  vp = (v0 + a0 * dt) + j0 * c2
__device__ __forceinline__ void predict_one(int k, const double4* __restrict__ pos, const double4* __restrict__ vel, const double4* __restrict__ acc,
                                            const double4* __restrict__ jerk, double4* __restrict__ xp, double4* __restrict__ vp, double dt, double c2,
                                            double c3) {
    const double4 x0 = pos[k], v0 = vel[k], a0 = acc[k], j0 = jerk[k];
    double4 x, v;
    x.x = ((x0.x + v0.x * dt) + a0.x * c2) + j0.x * c3;
    x.y = ((x0.y + v0.y * dt) + a0.y * c2) + j0.y * c3;
    x.z = ((x0.z + v0.z * dt) + a0.z * c2) + j0.z * c3;
    x.w = x0.w;
    v.x = (v0.x + a0.x * dt) + j0.x * c2;
    v.y = (v0.y + a0.y * dt) + j0.y * c2;
    v.z = (v0.z + a0.z * dt) + j0.z * c2;
    v.w = 0.0;
    xp[k] = x;
    vp[k] = v;
}

__global__ __launch_bounds__(256) void k_hm_predict(const double4* __restrict__ pos, const double4* __restrict__ vel,
                                                    const double4* __restrict__ acc, const double4* __restrict__ jerk,
                                                    const int* __restrict__ count, double4* __restrict__ xp, double4* __restrict__ vp,
                                                    HermiteCoef c) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= *count) return;
    predict_one(k, pos, vel, acc, jerk, xp, vp, c.dt, c.c2, c.c3);
}

// the corrector of body k, in place, and Bounds::contains (shared.rs:210-212: inclusive walls, a NaN is outside)
__device__ __forceinline__ void correct_one(int k, const double4 a1, const double4 j1, double4* __restrict__ pos, double4* __restrict__ vel,
                                            double4* __restrict__ acc, double4* __restrict__ jerk, unsigned char* __restrict__ keep,
                                            int* __restrict__ escaped, const HermiteCoef& c, const Bounds64& b) {
    const double4 x0 = pos[k], v0 = vel[k], a0 = acc[k], j0 = jerk[k];
    double4 v, x;
    v.x = (v0.x + (a0.x + a1.x) * c.h) + (j0.x - j1.x) * c.c12;
    v.y = (v0.y + (a0.y + a1.y) * c.h) + (j0.y - j1.y) * c.c12;
    v.z = (v0.z + (a0.z + a1.z) * c.h) + (j0.z - j1.z) * c.c12;
    v.w = 0.0;
    x.x = (x0.x + (v0.x + v.x) * c.h) + (a0.x - a1.x) * c.c12;
    x.y = (x0.y + (v0.y + v.y) * c.h) + (a0.y - a1.y) * c.c12;
    x.z = (x0.z + (v0.z + v.z) * c.h) + (a0.z - a1.z) * c.c12;
    x.w = x0.w;
    pos[k] = x;
    vel[k] = v;
    acc[k] = make_double4(a1.x, a1.y, a1.z, 0.0);
    jerk[k] = make_double4(j1.x, j1.y, j1.z, 0.0);
    const bool in = (x.x >= b.lo[0]) && (x.x <= b.hi[0]) && (x.y >= b.lo[1]) && (x.y <= b.hi[1]) && (x.z >= b.lo[2]) && (x.z <= b.hi[2]);
    keep[k] = in ? 1 : 0;
    if (!in) atomicAdd(escaped, 1);
}

__global__ __launch_bounds__(256) void k_hm_correct(const double4* __restrict__ a1, const double4* __restrict__ j1, double4* __restrict__ pos,
                                                    double4* __restrict__ vel, double4* __restrict__ acc, double4* __restrict__ jerk,
                                                    const int* __restrict__ count, unsigned char* __restrict__ keep,
                                                    int* __restrict__ escaped, HermiteCoef c, Bounds64 b) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= *count) return;
    correct_one(k, a1[k], j1[k], pos, vel, acc, jerk, keep, escaped, c, b);
}

// Vec::retain, one pass over many workgroups, in place: retain.h's look-back scan; what moves with a Hermite body is the
// jerk as a fourth array and, LV, its block-step level
constexpr int kTile = nbody::kCompactTile;   // (the block-step schedule below counts in the same tiles)

// LV: the block-step levels travel with the four arrays
template <bool LV>
__global__ __launch_bounds__(kTile) void k_hm_compact(double4* __restrict__ pos, double4* __restrict__ vel, double4* __restrict__ acc,
                                                      double4* __restrict__ jerk, const unsigned char* __restrict__ keep,
                                                      int* __restrict__ count, int* __restrict__ escaped,
                                                      unsigned long long* __restrict__ tile_state, int* __restrict__ epoch_p,
                                                      int* __restrict__ level) {
    if (*escaped == 0) return;
    double4 p = zero4(), v = p, a = p, j = p;
    int lv = 0;
    nbody::retain_tile(keep, count, escaped, tile_state, epoch_p,
                       [&](int k) { p = pos[k]; v = vel[k]; a = acc[k]; j = jerk[k]; if (LV) lv = level[k]; },
                       [&](int d) { pos[d] = p; vel[d] = v; acc[d] = a; jerk[d] = j; if (LV) level[d] = lv; });
}

// nbody_suggest_dt: min over the workgroup's live bodies of |a| / |j|, norms sqrt((x^2 + y^2) + z^2); bodies with |j| == 0
// (or a NaN in it) do not take part.  A minimum does not depend on the order it is taken in.
__global__ __launch_bounds__(256) void k_hm_min_ratio(const double4* __restrict__ acc, const double4* __restrict__ jerk,
                                                      const int* __restrict__ count, double* __restrict__ out) {
    __shared__ double part[4];
    const int k = blockIdx.x * 256 + threadIdx.x;
    double r = __builtin_inf();
    if (k < *count) {
        const double4 a = acc[k], j = jerk[k];
        const double na = __builtin_sqrt((a.x * a.x + a.y * a.y) + a.z * a.z);
        const double nj = __builtin_sqrt((j.x * j.x + j.y * j.y) + j.z * j.z);
        if (nj > 0.0) r = na / nj;
    }
    for (int off = 32; off > 0; off >>= 1) r = fmin(r, __shfl_down(r, off));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = r;
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = fmin(fmin(part[0], part[1]), fmin(part[2], part[3]));
}

// ------------------------------------------------------------------------------------------ strict F
constexpr int kStrictBlock = 256;
constexpr int kStrictTile = 256;   // positions and velocities: 16 KB of LDS

__global__ __launch_bounds__(kStrictBlock) void k_hm_strict(const double4* __restrict__ x, const double4* __restrict__ v,
                                                            const int* __restrict__ count, double4* __restrict__ out_a,
                                                            double4* __restrict__ out_j, double g, double eps2,
                                                            unsigned long long* __restrict__ inter) {
    __shared__ double4 tx[kStrictTile], tv[kStrictTile];
    const int tid = threadIdx.x;
    const int i = blockIdx.x * kStrictBlock + tid;
    const int n = *count;
    if (inter && blockIdx.x == 0 && tid == 0 && n > 0) atomicAdd(inter, (unsigned long long)n * (unsigned long long)(n - 1));
    const double4 pi = (i < n) ? x[i] : zero4();
    const double4 vi = (i < n) ? v[i] : zero4();
    double ax = 0.0, ay = 0.0, az = 0.0, jx = 0.0, jy = 0.0, jz = 0.0;
    for (int t0 = 0; t0 < n; t0 += kStrictTile) {
        const int cnt = min(kStrictTile, n - t0);
        __syncthreads();
        if (tid < cnt) { tx[tid] = x[t0 + tid]; tv[tid] = v[t0 + tid]; }
        __syncthreads();
        for (int t = 0; t < cnt; ++t) {
            if (t0 + t == i) continue;   // the i == j pair is never formed
            const double4 pj = tx[t], vj = tv[t];
            const double dx = pj.x - pi.x, dy = pj.y - pi.y, dz = pj.z - pi.z;
            const double dvx = vj.x - vi.x, dvy = vj.y - vi.y, dvz = vj.z - vi.z;
            const double r2 = ((dx * dx + dy * dy) + dz * dz) + eps2;
            const double rv = (dx * dvx + dy * dvy) + dz * dvz;
            const double w = (g * pj.w) / (r2 * __builtin_sqrt(r2));
            const double al = (3.0 * rv) / r2;
            ax += dx * w;
            ay += dy * w;
            az += dz * w;
            jx += (dvx - al * dx) * w;
            jy += (dvy - al * dy) * w;
            jz += (dvz - al * dz) * w;
        }
    }
    if (i < n) {
        out_a[i] = make_double4(ax, ay, az, 0.0);
        out_j[i] = make_double4(jx, jy, jz, 0.0);
    }
}

// ------------------------------------------------------------------------------------------ fast F, symmetric
template <int IPT>
struct Resident {   // 13 doubles a body; fully unrolled, so every member lives in registers
    double x[IPT], y[IPT], z[IPT], vx[IPT], vy[IPT], vz[IPT], m[IPT];
    double ax[IPT], ay[IPT], az[IPT], jx[IPT], jy[IPT], jz[IPT];
};
struct Traveller {
    double x, y, z, vx, vy, vz, m;
    double ax, ay, az, jx, jy, jz;
};

// IPT unordered pairs (resident q, traveller), B at a time and stage by stage so that no instruction waits on its predecessor
constexpr int kPairBatch = 4;   // (as pair_evals64 of kernels_bf64.hip; IPT = 4 stays below 256 registers: two waves per SIMD)
template <int IPT>
__device__ __forceinline__ void pair_evals_hm(Resident<IPT>& r, Traveller& t, double eps2) {
#pragma unroll
    for (int q0 = 0; q0 < IPT; q0 += kPairBatch) {
        constexpr int B = kPairBatch;
        double dx[B], dy[B], dz[B], wx[B], wy[B], wz[B], s[B], rv[B], sj[B];
#pragma unroll
        for (int u = 0; u < B; ++u) {
            dx[u] = t.x - r.x[q0 + u]; dy[u] = t.y - r.y[q0 + u]; dz[u] = t.z - r.z[q0 + u];
            wx[u] = t.vx - r.vx[q0 + u]; wy[u] = t.vy - r.vy[q0 + u]; wz[u] = t.vz - r.vz[q0 + u];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < B; ++u) { s[u] = fma(dx[u], dx[u], eps2); rv[u] = dx[u] * wx[u]; }
#pragma unroll
        for (int u = 0; u < B; ++u) { s[u] = fma(dy[u], dy[u], s[u]); rv[u] = fma(dy[u], wy[u], rv[u]); }
#pragma unroll
        for (int u = 0; u < B; ++u) { s[u] = fma(dz[u], dz[u], s[u]); rv[u] = fma(dz[u], wz[u], rv[u]); }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < B; ++u) s[u] = rsqrt(s[u]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < B; ++u) sj[u] = s[u] * s[u];              // rinv^2
#pragma unroll
        for (int u = 0; u < B; ++u) s[u] = sj[u] * s[u];              // rinv^3
#pragma unroll
        for (int u = 0; u < B; ++u) rv[u] = (-3.0 * sj[u]) * rv[u];   // -3 (d.w) / q
#pragma unroll
        for (int u = 0; u < B; ++u) {                                 // u = w - 3 (d.w)/q d: shared by both sides
            wx[u] = fma(rv[u], dx[u], wx[u]);
            wy[u] = fma(rv[u], dy[u], wy[u]);
            wz[u] = fma(rv[u], dz[u], wz[u]);
        }
#pragma unroll
        for (int u = 0; u < B; ++u) sj[u] = t.m * s[u];               // what the traveller does to the resident body
#pragma unroll
        for (int u = 0; u < B; ++u) s[u] = r.m[q0 + u] * s[u];        // what the resident body does to the traveller
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < B; ++u) {
            r.ax[q0 + u] = fma(dx[u], sj[u], r.ax[q0 + u]);
            r.ay[q0 + u] = fma(dy[u], sj[u], r.ay[q0 + u]);
            r.az[q0 + u] = fma(dz[u], sj[u], r.az[q0 + u]);
            r.jx[q0 + u] = fma(wx[u], sj[u], r.jx[q0 + u]);
            r.jy[q0 + u] = fma(wy[u], sj[u], r.jy[q0 + u]);
            r.jz[q0 + u] = fma(wz[u], sj[u], r.jz[q0 + u]);
            t.ax = fma(-dx[u], s[u], t.ax);
            t.ay = fma(-dy[u], s[u], t.ay);
            t.az = fma(-dz[u], s[u], t.az);
            t.jx = fma(-wx[u], s[u], t.jx);
            t.jy = fma(-wy[u], s[u], t.jy);
            t.jz = fma(-wz[u], s[u], t.jz);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

// 4 waves per workgroup; wave gw = a * K + part is slice `part` of resident set a (k_bf64_sym's decomposition)
template <int IPT, int ROT>
__global__ __launch_bounds__(256) void k_hm_sym(const double4* __restrict__ pos, const double4* __restrict__ vel, const int* __restrict__ count,
                                                int A, int K, int sym_sets, double4* __restrict__ planes, size_t plane_stride, size_t jerk_off,
                                                double eps2) {
    __shared__ double4 tile[ROT == 0 ? 4 : 1][2][64];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int gw = blockIdx.x * 4 + wv;
    if (gw >= A * K) return;
    const int a = gw / K, part = gw - a * K;
    const int n = *count;
    const int Cn = A * IPT;                       // chunks in the padded body array
    const int L = IPT * sym_sets;                 // chunk visits of a set
    const int k0 = int((long long)L * part / K), k1 = int((long long)L * (part + 1) / K);
    const int src1 = ((lane + 63) & 63) * 4;      // ds_bpermute address: take from the lane below
    // eps2 in a VGPR (kernels_bf_sym.hip: an SGPR operand makes the compiler drain all LDS traffic every step)
    double eps2v = eps2;
    asm volatile("" : "+v"(eps2v));

    Resident<IPT> r;
#pragma unroll
    for (int q = 0; q < IPT; ++q) {
        const int i = (a * IPT + q) * 64 + lane;
        const double4 p = (i < n) ? pos[i] : pad_body();
        const double4 v = (i < n) ? vel[i] : zero4();
        r.x[q] = p.x; r.y[q] = p.y; r.z[q] = p.z; r.m[q] = p.w;
        r.vx[q] = v.x; r.vy[q] = v.y; r.vz[q] = v.z;
        r.ax[q] = r.ay[q] = r.az[q] = r.jx[q] = r.jy[q] = r.jz[q] = 0.0;
    }
    auto chunk_of = [&](int k) {
        int c = (a + 1) * IPT + k;
        if (c >= Cn) c -= Cn;
        return c;
    };
    double4 nxt_p = pad_body(), nxt_v = zero4();
    auto load_chunk = [&](int k) {
        const int j = chunk_of(k) * 64 + lane;
        nxt_p = (j < n) ? pos[j] : pad_body();
        nxt_v = (j < n) ? vel[j] : zero4();
    };
    if (k0 < k1) load_chunk(k0);
    for (int k = k0; k < k1; ++k) {
        const double4 cur_p = nxt_p, cur_v = nxt_v;
        if (k + 1 < k1) load_chunk(k + 1);
        Traveller t;
        t.ax = t.ay = t.az = t.jx = t.jy = t.jz = 0.0;
        // at step s lane l meets the body that started in lane (l - s) & 63, whose accumulators it holds
        if (ROT == 0) {
            tile[wv][0][lane] = cur_p;   // the wave's own tile: its LDS operations complete in program order
            tile[wv][1][lane] = cur_v;
            for (int s = 0; s < 64; ++s) {
                const double4 pj = tile[wv][0][(lane - s) & 63];
                const double4 vj = tile[wv][1][(lane - s) & 63];
                t.x = pj.x; t.y = pj.y; t.z = pj.z; t.m = pj.w;
                t.vx = vj.x; t.vy = vj.y; t.vz = vj.z;
                pair_evals_hm<IPT>(r, t, eps2v);
                t.ax = rot64(t.ax, src1); t.ay = rot64(t.ay, src1); t.az = rot64(t.az, src1);
                t.jx = rot64(t.jx, src1); t.jy = rot64(t.jy, src1); t.jz = rot64(t.jz, src1);
            }
        } else {
            t.x = cur_p.x; t.y = cur_p.y; t.z = cur_p.z; t.m = cur_p.w;
            t.vx = cur_v.x; t.vy = cur_v.y; t.vz = cur_v.z;
            for (int s = 0; s < 64; ++s) {
                // the next step's body is requested before this step's arithmetic: the crossbar latency hides behind it
                const double x1 = rot64(t.x, src1), y1 = rot64(t.y, src1), z1 = rot64(t.z, src1), m1 = rot64(t.m, src1);
                const double vx1 = rot64(t.vx, src1), vy1 = rot64(t.vy, src1), vz1 = rot64(t.vz, src1);
                pair_evals_hm<IPT>(r, t, eps2v);
                t.ax = rot64(t.ax, src1); t.ay = rot64(t.ay, src1); t.az = rot64(t.az, src1);
                t.jx = rot64(t.jx, src1); t.jy = rot64(t.jy, src1); t.jz = rot64(t.jz, src1);
                t.x = x1; t.y = y1; t.z = z1; t.m = m1; t.vx = vx1; t.vy = vy1; t.vz = vz1;
            }
        }
        const int d = k / IPT + 1;   // set distance 1..sym_sets
        const size_t row = size_t(d - 1) * plane_stride + size_t(chunk_of(k)) * 64 + lane;
        planes[row] = make_double4(t.ax, t.ay, t.az, 0.0);
        planes[jerk_off + row] = make_double4(t.jx, t.jy, t.jz, 0.0);
    }
    double4* __restrict__ out = planes + size_t(sym_sets + part) * plane_stride;
#pragma unroll
    for (int q = 0; q < IPT; ++q) {
        const size_t row = size_t(a * IPT + q) * 64 + lane;
        out[row] = make_double4(r.ax[q], r.ay[q], r.az[q], 0.0);
        out[jerk_off + row] = make_double4(r.jx[q], r.jy[q], r.jz[q], 0.0);
    }
}

// ------------------------------------------------------------------------------------------ fast F, one-sided
// what body j does to body i, one pair (k_hm_os, k_hm_act); self: the i == j pair, which is never formed (with g_soft = 0 its
// rsqrt is inf)
__device__ __forceinline__ void one_pair_hm(const double4 pi, const double4 vi, const double4 pj, const double4 vj, bool self, double eps2,
                                            double& ax, double& ay, double& az, double& jx, double& jy, double& jz) {
    const double dx = pj.x - pi.x, dy = pj.y - pi.y, dz = pj.z - pi.z;
    double wx = vj.x - vi.x, wy = vj.y - vi.y, wz = vj.z - vi.z;
    const double q = fma(dz, dz, fma(dy, dy, fma(dx, dx, eps2)));
    const double rv = fma(dz, wz, fma(dy, wy, dx * wx));
    double rinv = rsqrt(q);
    rinv = self ? 0.0 : rinv;
    const double rinv2 = rinv * rinv;
    const double nal = (-3.0 * rinv2) * rv;
    const double sj = pj.w * (rinv2 * rinv);
    wx = fma(nal, dx, wx);
    wy = fma(nal, dy, wy);
    wz = fma(nal, dz, wz);
    ax = fma(dx, sj, ax);
    ay = fma(dy, sj, ay);
    az = fma(dz, sj, az);
    jx = fma(wx, sj, jx);
    jy = fma(wy, sj, jy);
    jz = fma(wz, sj, jz);
}

// 4 waves per workgroup; wave gw = group * K + slice: bodies group*64 + lane against slice `slice` of the partner list
// (MODE 0: every own body; MODE 1: the own set and, for even A, the opposite set).  Output: plane `slice`, rows
// group*64 .. group*64+63 (every row, padding included).
template <int MODE>
__global__ __launch_bounds__(256) void k_hm_os(const double4* __restrict__ pos, const double4* __restrict__ vel, const int* __restrict__ count,
                                               int set_size, int A, int groups, int K, double4* __restrict__ planes, size_t plane_stride,
                                               size_t jerk_off, double eps2) {
    __shared__ double4 tile[4][2][64];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int gw = blockIdx.x * 4 + wv;
    if (gw >= groups * K) return;
    const int group = gw / K, slice = gw - group * K;
    const int n = *count;
    const int i = group * 64 + lane;
    const double4 pi = (i < n) ? pos[i] : pad_body();
    const double4 vi = (i < n) ? vel[i] : zero4();
    const int a = (group * 64) / set_size;       // (MODE 1: the set of all 64 bodies of the group)
    double eps2v = eps2;
    asm volatile("" : "+v"(eps2v));
    const int nw = MODE == 0 ? 1 : ((A % 2 == 0 && A > 1) ? 2 : 1);
    int wlo[2] = {0, 0}, whi[2] = {0, 0};
    long long R = 0;
    for (int w = 0; w < nw; ++w) {
        if (MODE == 0) { wlo[w] = 0; whi[w] = n; }
        else {
            int set = (w == 0) ? a : a + A / 2;
            if (set >= A) set -= A;
            wlo[w] = min(n, set * set_size);
            whi[w] = min(n, wlo[w] + set_size);
        }
        R += whi[w] - wlo[w];
    }
    const long long r0 = R * slice / K, r1 = R * (slice + 1) / K;
    double ax = 0.0, ay = 0.0, az = 0.0, jx = 0.0, jy = 0.0, jz = 0.0;
    long long first = 0;   // index of the window's first body in the concatenated partner list
    for (int w = 0; w < nw; ++w) {
        const int len = whi[w] - wlo[w];
        const long long lo = max(r0, first), hi = min(r1, first + len);
        if (lo < hi) {
            const double4* __restrict__ ps = pos + wlo[w];   // ps[c - first]: partner c
            const double4* __restrict__ vs = vel + wlo[w];
            const long long self = (i >= wlo[w] && i < whi[w]) ? first + (i - wlo[w]) : -1;   // the own body's place in the list
            double4 nxt_p = pad_body(), nxt_v = zero4();
            if (lo + lane < hi) { nxt_p = ps[lo + lane - first]; nxt_v = vs[lo + lane - first]; }
            for (long long c0 = lo; c0 < hi; c0 += 64) {
                tile[wv][0][lane] = nxt_p;   // the wave's own tile: its LDS operations complete in program order
                tile[wv][1][lane] = nxt_v;
                if (c0 + 64 + lane < hi) { nxt_p = ps[c0 + 64 + lane - first]; nxt_v = vs[c0 + 64 + lane - first]; }
                const int cnt = int(min(64LL, hi - c0));
                for (int t = 0; t < cnt; ++t) {
                    const double4 pj = tile[wv][0][t];   // wave-uniform address: an LDS broadcast
                    const double4 vj = tile[wv][1][t];
                    one_pair_hm(pi, vi, pj, vj, c0 + t == self, eps2v, ax, ay, az, jx, jy, jz);
                }
            }
        }
        first += len;
    }
    const size_t row = size_t(slice) * plane_stride + i;
    planes[row] = make_double4(ax, ay, az, 0.0);
    planes[jerk_off + row] = make_double4(jx, jy, jz, 0.0);
}

// the planes added in a fixed order, times g; CORRECT: the corrector (k_hm_correct's arithmetic) rides along
template <bool CORRECT>
__global__ __launch_bounds__(256) void k_hm_reduce(const double4* __restrict__ planes, int n_planes, size_t plane_stride, size_t jerk_off,
                                                   const int* __restrict__ count, double g, double4* __restrict__ out_a,
                                                   double4* __restrict__ out_j, double4* __restrict__ pos, double4* __restrict__ vel,
                                                   double4* __restrict__ acc, double4* __restrict__ jerk, unsigned char* __restrict__ keep,
                                                   int* __restrict__ escaped, HermiteCoef c, Bounds64 b, unsigned long long* __restrict__ inter) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int n = *count;
    if (inter && i == 0 && n > 0) atomicAdd(inter, (unsigned long long)n * (unsigned long long)(n - 1));
    if (i >= n) return;
    double4 a1, j1;
    plane_sum<2>(planes, n_planes, plane_stride, jerk_off, i, g, a1, j1);
    if (CORRECT) correct_one(i, a1, j1, pos, vel, acc, jerk, keep, escaped, c, b);
    else { out_a[i] = a1; out_j[i] = j1; }
}

// ------------------------------------------------------------------------------------------ block individual time steps
// One macro step of T = 2^L ticks (include/nbody_hip.h "block steps").  Body i sits at tick tau[i] with a step of T >> level[i]
// ticks.  A block step: k_hmb_min (tau* = the earliest due tick), k_hmb_count + k_hmb_list (the due bodies' indices in
// ascending order, and every body predicted to tau*), k_hm_act / k_hm_act_strict (F of the listed bodies against all n
// predicted ones), k_hmb_finish (planes, corrector, step criterion, new level).  No kernel hands data to another workgroup
// of its own launch: tau*, the per-tile counts and the list cross launch boundaries only.
constexpr int kNever = 0x7f7f7f7f;   // (what the host's memset writes into BlockDev::smin)

// the level a step of |dt| 2^-l must reach to be <= dtc (a NaN dtc gives 0, dtc == 0 gives max_level)
__device__ __forceinline__ int level_for(double dtc, double abs_dt, int max_level) {
    int l = 0;
    double s = abs_dt;
    while (s > dtc && l < max_level) { s *= 0.5; ++l; }
    return l;
}
__device__ __forceinline__ double norm3(double x, double y, double z) { return __builtin_sqrt((x * x + y * y) + z * z); }

// start levels from the held derivatives: dtc = eta (|a| / |j|)
__global__ __launch_bounds__(256) void k_hmb_start(const double4* __restrict__ acc, const double4* __restrict__ jerk, const int* __restrict__ count,
                                                   int* __restrict__ level, double eta, double abs_dt, int max_level) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= *count) return;
    const double4 a = acc[k], j = jerk[k];
    const double dtc = eta * (norm3(a.x, a.y, a.z) / norm3(j.x, j.y, j.z));
    level[k] = level_for(dtc, abs_dt, max_level);
}

// smin[slot] = min_i (tau_i + s_i); the other slot is re-armed for the next block step
__global__ __launch_bounds__(256) void k_hmb_min(const int* __restrict__ tau, const int* __restrict__ level, const int* __restrict__ count, int T,
                                                 int* __restrict__ smin, int slot) {
    __shared__ int part[4];
    const int k = blockIdx.x * 256 + threadIdx.x;
    int r = kNever;
    if (k < *count) r = tau[k] + (T >> level[k]);
    for (int off = 32; off > 0; off >>= 1) r = min(r, __shfl_down(r, off));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = r;
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicMin(smin + slot, min(min(part[0], part[1]), min(part[2], part[3])));   // (a minimum does not depend on the order)
        if (blockIdx.x == 0) smin[slot ^ 1] = kNever;
    }
}

// due bodies of every 1024-body tile
__global__ __launch_bounds__(kTile) void k_hmb_count(const int* __restrict__ tau, const int* __restrict__ level, const int* __restrict__ count, int T,
                                                     const int* __restrict__ smin, int slot, int* __restrict__ tile_count) {
    __shared__ int wave_total[16];
    const int tid = threadIdx.x;
    const int k = blockIdx.x * kTile + tid;
    const bool due = (k < *count) && (tau[k] + (T >> level[k]) == smin[slot]);
    const unsigned long long m = __ballot(due);
    if ((tid & 63) == 0) wave_total[tid >> 6] = __popcll(m);
    __syncthreads();
    if (tid == 0) {
        int total = 0;
        for (int w = 0; w < 16; ++w) total += wave_total[w];
        tile_count[blockIdx.x] = total;
    }
}

// the due bodies' indices, ascending, into list; every body predicted to tau* (predict_one with the body's own
// dp = f64(tau* - tau_i) tick and hermite_coef's c2, c3); the last tile reports {tau*, how many are due}
__global__ __launch_bounds__(kTile) void k_hmb_list(const double4* __restrict__ pos, const double4* __restrict__ vel, const double4* __restrict__ acc,
                                                    const double4* __restrict__ jerk, const int* __restrict__ tau, const int* __restrict__ level,
                                                    const int* __restrict__ count, int T, double tick, const int* __restrict__ smin, int slot,
                                                    const int* __restrict__ tile_count, int* __restrict__ list, int* __restrict__ sched,
                                                    double4* __restrict__ xp, double4* __restrict__ vp) {
    __shared__ int wave_total[16];
    __shared__ int red[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tile = blockIdx.x;
    const int n = *count;
    const int tstar = smin[slot];
    const int k = tile * kTile + tid;
    bool due = false;
    if (k < n) {
        const int tk = tau[k];
        due = tk + (T >> level[k]) == tstar;
        const double dp = double(tstar - tk) * tick;
        const double c2 = (dp * dp) * 0.5, c3 = ((dp * dp) * dp) / 6.0;
        predict_one(k, pos, vel, acc, jerk, xp, vp, dp, c2, c3);
    }
    int before_tiles = 0;   // due bodies of the tiles below this one: integer sums, any order
    for (int t = tid; t < tile; t += kTile) before_tiles += tile_count[t];
    for (int off = 32; off > 0; off >>= 1) before_tiles += __shfl_down(before_tiles, off);
    const unsigned long long m = __ballot(due);
    if (lane == 0) { wave_total[wave] = __popcll(m); red[wave] = before_tiles; }
    __syncthreads();
    int excl = 0, before = 0, total = 0;
    for (int w = 0; w < 16; ++w) {
        excl += red[w];
        if (w < wave) before += wave_total[w];
        total += wave_total[w];
    }
    if (due) list[excl + before + __popcll(m & ((1ull << lane) - 1ull))] = k;
    if (tid == 0 && tile == int(gridDim.x) - 1) { sched[0] = tstar; sched[1] = excl + total; }
}

// NBODY_MATH_FAST: F of the listed bodies.  4 waves per workgroup; wave gw = group * K + slice: the bodies list[group*64 + lane]
// against partners [n slice / K, n (slice + 1) / K) of ALL n bodies of (x, v), staged 64 at a time through the wave's own LDS
// tile (k_hm_os<0>'s loop; one_pair_hm).  Output: plane `slice`, rows group*64 .. group*64+63: every row of every plane is
// written exactly once, padding rows and empty slices included.
__global__ __launch_bounds__(256) void k_hm_act(const double4* __restrict__ x, const double4* __restrict__ v, const int* __restrict__ count,
                                                const int* __restrict__ list, const int* __restrict__ n_act_p, int groups, int K,
                                                double4* __restrict__ planes, size_t plane_stride, size_t jerk_off, double eps2) {
    __shared__ double4 tile[4][2][64];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int gw = blockIdx.x * 4 + wv;
    if (gw >= groups * K) return;
    const int group = gw / K, slice = gw - group * K;
    const int n = *count;
    const int p = group * 64 + lane;
    const int i = (p < *n_act_p) ? list[p] : -1;   // (-1: a padding lane; no partner has that index)
    const double4 pi = (i >= 0) ? x[i] : pad_body();
    const double4 vi = (i >= 0) ? v[i] : zero4();
    double eps2v = eps2;
    asm volatile("" : "+v"(eps2v));
    const int lo = int((long long)n * slice / K), hi = int((long long)n * (slice + 1) / K);
    double ax = 0.0, ay = 0.0, az = 0.0, jx = 0.0, jy = 0.0, jz = 0.0;
    double4 nxt_p = pad_body(), nxt_v = zero4();
    if (lo + lane < hi) { nxt_p = x[lo + lane]; nxt_v = v[lo + lane]; }
    for (int c0 = lo; c0 < hi; c0 += 64) {
        tile[wv][0][lane] = nxt_p;   // the wave's own tile: its LDS operations complete in program order
        tile[wv][1][lane] = nxt_v;
        if (c0 + 64 + lane < hi) { nxt_p = x[c0 + 64 + lane]; nxt_v = v[c0 + 64 + lane]; }
        const int cnt = min(64, hi - c0);
        for (int t = 0; t < cnt; ++t) {
            const double4 pj = tile[wv][0][t];   // wave-uniform address: an LDS broadcast
            const double4 vj = tile[wv][1][t];
            one_pair_hm(pi, vi, pj, vj, c0 + t == i, eps2v, ax, ay, az, jx, jy, jz);
        }
    }
    const size_t row = size_t(slice) * plane_stride + size_t(p);
    planes[row] = make_double4(ax, ay, az, 0.0);
    planes[jerk_off + row] = make_double4(jx, jy, jz, 0.0);
}

// NBODY_MATH_STRICT: one listed body per lane, partners in ascending index order (k_hm_strict's expressions); row p of the
// outputs belongs to list[p]
__global__ __launch_bounds__(kStrictBlock) void k_hm_act_strict(const double4* __restrict__ x, const double4* __restrict__ v,
                                                                const int* __restrict__ count, const int* __restrict__ list,
                                                                const int* __restrict__ n_act_p, double4* __restrict__ out_a,
                                                                double4* __restrict__ out_j, double g, double eps2) {
    __shared__ double4 tx[kStrictTile], tv[kStrictTile];
    const int tid = threadIdx.x;
    const int p = blockIdx.x * kStrictBlock + tid;
    const int n = *count;
    const int i = (p < *n_act_p) ? list[p] : -1;
    const double4 pi = (i >= 0) ? x[i] : zero4();
    const double4 vi = (i >= 0) ? v[i] : zero4();
    double ax = 0.0, ay = 0.0, az = 0.0, jx = 0.0, jy = 0.0, jz = 0.0;
    for (int t0 = 0; t0 < n; t0 += kStrictTile) {
        const int cnt = min(kStrictTile, n - t0);
        __syncthreads();
        if (tid < cnt) { tx[tid] = x[t0 + tid]; tv[tid] = v[t0 + tid]; }
        __syncthreads();
        for (int t = 0; t < cnt; ++t) {
            if (t0 + t == i) continue;   // the i == j pair is never formed
            const double4 pj = tx[t], vj = tv[t];
            const double dx = pj.x - pi.x, dy = pj.y - pi.y, dz = pj.z - pi.z;
            const double dvx = vj.x - vi.x, dvy = vj.y - vi.y, dvz = vj.z - vi.z;
            const double r2 = ((dx * dx + dy * dy) + dz * dz) + eps2;
            const double rv = (dx * dvx + dy * dvy) + dz * dvz;
            const double w = (g * pj.w) / (r2 * __builtin_sqrt(r2));
            const double al = (3.0 * rv) / r2;
            ax += dx * w;
            ay += dy * w;
            az += dz * w;
            jx += (dvx - al * dx) * w;
            jy += (dvy - al * dy) * w;
            jz += (dvz - al * dz) * w;
        }
    }
    if (i >= 0) {
        out_a[p] = make_double4(ax, ay, az, 0.0);
        out_j[p] = make_double4(jx, jy, jz, 0.0);
    }
}

// what a block step does to its due bodies, one per lane: (a1, j1) from the K planes added in a fixed order, times g (PLANES)
// or from row p of (in_a, in_j); STEP: the corrector with the body's own h = f64(s_i) tick, the a2 / a3 step criterion, the new
// level, tau_i = tau* -- the due body's state is read and written once; else (a1, j1) go to row p of (out_a, out_j)
template <bool PLANES, bool STEP>
__global__ __launch_bounds__(256) void k_hmb_finish(const double4* __restrict__ planes, int n_planes, size_t plane_stride, size_t jerk_off,
                                                    const double4* __restrict__ in_a, const double4* __restrict__ in_j, double4* __restrict__ out_a,
                                                    double4* __restrict__ out_j, const int* __restrict__ count, const int* __restrict__ list,
                                                    const int* __restrict__ sched, double g, double4* __restrict__ pos, double4* __restrict__ vel,
                                                    double4* __restrict__ acc, double4* __restrict__ jerk, unsigned char* __restrict__ keep,
                                                    int* __restrict__ escaped, int* __restrict__ tau, int* __restrict__ level, int T, int max_level,
                                                    double tick, double abs_dt, double eta, Bounds64 b, unsigned long long* __restrict__ inter) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    const int n_act = sched[1];
    if (STEP && inter && p == 0 && n_act > 0) atomicAdd(inter, (unsigned long long)n_act * (unsigned long long)(*count - 1));
    if (p >= n_act) return;
    double4 a1, j1;
    if (PLANES) {
        plane_sum<2>(planes, n_planes, plane_stride, jerk_off, p, g, a1, j1);
    } else {
        a1 = in_a[p];
        j1 = in_j[p];
    }
    if (!STEP) { out_a[p] = a1; out_j[p] = j1; return; }
    const int i = list[p];
    const int tstar = sched[0];
    const int l = level[i];
    const double h = double(T >> l) * tick;
    const double4 a0 = acc[i], j0 = jerk[i];
    HermiteCoef c{};
    c.h = h * 0.5;
    c.c12 = (h * h) / 12.0;
    correct_one(i, a1, j1, pos, vel, acc, jerk, keep, escaped, c, b);
    const double h2 = h * h, h3 = h2 * h, h6 = h * 6.0;
    const double dax = a0.x - a1.x, day = a0.y - a1.y, daz = a0.z - a1.z;
    const double a3x = (dax * 12.0 + (j0.x + j1.x) * h6) / h3;
    const double a3y = (day * 12.0 + (j0.y + j1.y) * h6) / h3;
    const double a3z = (daz * 12.0 + (j0.z + j1.z) * h6) / h3;
    const double a2x = ((dax * -6.0 - (j0.x * 4.0 + j1.x * 2.0) * h) / h2) + a3x * h;   // the second derivative at the END of the step
    const double a2y = ((day * -6.0 - (j0.y * 4.0 + j1.y * 2.0) * h) / h2) + a3y * h;
    const double a2z = ((daz * -6.0 - (j0.z * 4.0 + j1.z * 2.0) * h) / h2) + a3z * h;
    const double na = norm3(a1.x, a1.y, a1.z), nj = norm3(j1.x, j1.y, j1.z);
    const double n2 = norm3(a2x, a2y, a2z), n3 = norm3(a3x, a3y, a3z);
    const double dtc = __builtin_sqrt(eta * ((na * n2 + nj * nj) / (nj * n3 + n2 * n2)));
    const int want = level_for(dtc, abs_dt, max_level);
    int nl = l;
    if (want > l) nl = want;                                                   // any finer step is commensurate
    else if (want < l && l > 0 && (tstar % (T >> (l - 1))) == 0) nl = l - 1;   // a step doubles once, and only on its own grid
    level[i] = nl;
    tau[i] = tstar;
}

inline int blocks_for(long long n, int per) { return int((n + per - 1) / per); }

}  // namespace

// ----------------------------------------------------------------------------------- host side
void launch_hm_predict(hipStream_t s, const Dev& d, const HermiteDev& hd, int n_upper, const HermiteCoef& c) {
    if (n_upper <= 0) return;
    hipLaunchKernelGGL(k_hm_predict, dim3(blocks_for(n_upper, 256)), dim3(256), 0, s, d.own_pos(), d.vel, d.acc, hd.jerk, d.own_count(), hd.xp, hd.vp, c);
}

void launch_hm_strict(hipStream_t s, const Dev& d, const double4* x, const double4* v, double4* out_a, double4* out_j, int n_upper, double g, double eps2) {
    if (n_upper <= 0) return;
    hipLaunchKernelGGL(k_hm_strict, dim3(blocks_for(n_upper, kStrictBlock)), dim3(kStrictBlock), 0, s, x, v, d.own_count(), out_a, out_j, g, eps2, d.inter);
}

void launch_hm_correct(hipStream_t s, const Dev& d, const HermiteDev& hd, int n_upper, const HermiteCoef& c, const Bounds64& b) {
    if (n_upper <= 0) return;
    hipLaunchKernelGGL(k_hm_correct, dim3(blocks_for(n_upper, 256)), dim3(256), 0, s, hd.a1, hd.j1, d.own_pos(), d.vel, d.acc, hd.jerk, d.own_count(), d.keep,
                       d.escaped, c, b);
}

void launch_hm_compact(hipStream_t s, const Dev& d, const HermiteDev& hd, int n_upper, int* level) {
    if (n_upper <= 0) return;
    if (level)
        hipLaunchKernelGGL(k_hm_compact<true>, dim3(blocks_for(n_upper, kTile)), dim3(kTile), 0, s, d.own_pos(), d.vel, d.acc, hd.jerk, d.keep, d.own_count(),
                           d.escaped, d.tile_state, d.epoch, level);
    else
        hipLaunchKernelGGL(k_hm_compact<false>, dim3(blocks_for(n_upper, kTile)), dim3(kTile), 0, s, d.own_pos(), d.vel, d.acc, hd.jerk, d.keep, d.own_count(),
                           d.escaped, d.tile_state, d.epoch, level);
}

int launch_hm_min_ratio(hipStream_t s, const Dev& d, const HermiteDev& hd, int n_upper) {
    if (n_upper <= 0) return 0;
    const int blocks = blocks_for(n_upper, 256);
    hipLaunchKernelGGL(k_hm_min_ratio, dim3(blocks), dim3(256), 0, s, d.acc, hd.jerk, d.own_count(), hd.ratio);
    return blocks;
}

void launch_hm_sym(hipStream_t s, const Dev& d, const Bf64Plan& p, const double4* x, const double4* v, double4* planes, double eps2) {
    if (!p.sym || p.sym_sets <= 0) return;
    const dim3 grid(blocks_for((long long)p.A * p.K, 4)), block(256);
    const size_t joff = size_t(p.n_planes) * p.n_pad;
#define HMSYM(I, R) hipLaunchKernelGGL((k_hm_sym<I, R>), grid, block, 0, s, x, v, d.own_count(), p.A, p.K, p.sym_sets, planes, p.n_pad, joff, eps2)
    if (p.ipt == 8) { if (p.rot) HMSYM(8, 1); else HMSYM(8, 0); }
    else { if (p.rot) HMSYM(4, 1); else HMSYM(4, 0); }   // (hermite_ipt() yields nothing else)
#undef HMSYM
}

void launch_hm_own(hipStream_t s, const Dev& d, const Bf64Plan& p, const double4* x, const double4* v, double4* planes, double eps2) {
    double4* out = planes + size_t(p.sym_sets + p.K) * p.n_pad;
    const dim3 grid(blocks_for((long long)p.groups * p.k_own, 4)), block(256);
    const size_t joff = size_t(p.n_planes) * p.n_pad;
    if (p.sym)
        hipLaunchKernelGGL(k_hm_os<1>, grid, block, 0, s, x, v, d.own_count(), 64 * p.ipt, p.A, p.groups, p.k_own, out, p.n_pad, joff, eps2);
    else
        hipLaunchKernelGGL(k_hm_os<0>, grid, block, 0, s, x, v, d.own_count(), 64, 1, p.groups, p.k_own, out, p.n_pad, joff, eps2);
}

void launch_hm_reduce(hipStream_t s, const Dev& d, const HermiteDev& hd, const Bf64Plan& p, const double4* planes, int n_upper, double g,
                      double4* out_a, double4* out_j, const HermiteCoef* c, const Bounds64& b) {
    if (n_upper <= 0) return;
    const dim3 grid(blocks_for(n_upper, 256)), block(256);
    const size_t joff = size_t(p.n_planes) * p.n_pad;
    if (c)
        hipLaunchKernelGGL(k_hm_reduce<true>, grid, block, 0, s, planes, p.n_planes, p.n_pad, joff, d.own_count(), g, out_a, out_j, d.own_pos(), d.vel, d.acc,
                           hd.jerk, d.keep, d.escaped, *c, b, d.inter);
    else
        hipLaunchKernelGGL(k_hm_reduce<false>, grid, block, 0, s, planes, p.n_planes, p.n_pad, joff, d.own_count(), g, out_a, out_j, d.own_pos(), d.vel, d.acc,
                           hd.jerk, d.keep, d.escaped, HermiteCoef{}, b, d.inter);
}

// ----------------------------------------------------------------------------------- block steps, host side
void launch_hmb_start_levels(hipStream_t s, const Dev& d, const HermiteDev& hd, const BlockDev& bd, int n_upper, double eta, double abs_dt,
                             int max_level) {
    if (n_upper <= 0) return;
    hipLaunchKernelGGL(k_hmb_start, dim3(blocks_for(n_upper, 256)), dim3(256), 0, s, d.acc, hd.jerk, d.own_count(), bd.level, eta, abs_dt, max_level);
}

void launch_hmb_schedule(hipStream_t s, const Dev& d, const HermiteDev& hd, const BlockDev& bd, int n_upper, int T, double tick, int slot) {
    if (n_upper <= 0) return;
    const int tiles = blocks_for(n_upper, kTile);
    hipLaunchKernelGGL(k_hmb_min, dim3(blocks_for(n_upper, 256)), dim3(256), 0, s, bd.tau, bd.level, d.own_count(), T, bd.smin, slot);
    hipLaunchKernelGGL(k_hmb_count, dim3(tiles), dim3(kTile), 0, s, bd.tau, bd.level, d.own_count(), T, bd.smin, slot, bd.tile_count);
    hipLaunchKernelGGL(k_hmb_list, dim3(tiles), dim3(kTile), 0, s, d.own_pos(), d.vel, d.acc, hd.jerk, bd.tau, bd.level, d.own_count(), T, tick, bd.smin, slot,
                       bd.tile_count, bd.list, bd.sched, hd.xp, hd.vp);
}

HmActPlan make_hm_act_plan(int n_act, int n) {
    HmActPlan p;
    const int want = nbody::tuning().bf64_waves > 0 ? nbody::tuning().bf64_waves : 2048;
    p.groups = blocks_for(n_act, 64);
    p.K = std::max(1, std::min(want / std::max(1, p.groups), blocks_for(n, 64)));   // (a slice holds a 64-partner tile or more)
    return p;
}

size_t hm_act_plane_rows(int cap) {
    const int want = nbody::tuning().bf64_waves > 0 ? nbody::tuning().bf64_waves : 2048;
    return size_t(std::max(want, blocks_for(cap, 64))) * 64;   // K groups <= max(want, groups)
}

void launch_hm_act(hipStream_t s, const Dev& d, const BlockDev& bd, const HmActPlan& p, const double4* x, const double4* v, double eps2) {
    if (p.groups <= 0) return;
    const size_t stride = size_t(p.groups) * 64;
    hipLaunchKernelGGL(k_hm_act, dim3(blocks_for((long long)p.groups * p.K, 4)), dim3(256), 0, s, x, v, d.own_count(), bd.list, bd.sched + 1, p.groups, p.K,
                       bd.planes, stride, size_t(p.K) * stride, eps2);
}

void launch_hm_act_strict(hipStream_t s, const Dev& d, const HermiteDev& hd, const BlockDev& bd, int n_act, const double4* x, const double4* v,
                          double g, double eps2) {
    if (n_act <= 0) return;
    hipLaunchKernelGGL(k_hm_act_strict, dim3(blocks_for(n_act, kStrictBlock)), dim3(kStrictBlock), 0, s, x, v, d.own_count(), bd.list, bd.sched + 1, hd.a1,
                       hd.j1, g, eps2);
}

void launch_hmb_finish(hipStream_t s, const Dev& d, const HermiteDev& hd, const BlockDev& bd, const HmActPlan* p, int n_act, double g, int T,
                       int max_level, double tick, double abs_dt, double eta, const Bounds64& b) {
    if (n_act <= 0) return;
    const dim3 grid(blocks_for(n_act, 256)), block(256);
    const size_t stride = p ? size_t(p->groups) * 64 : 0;
#define HMFIN(PL) hipLaunchKernelGGL((k_hmb_finish<PL, true>), grid, block, 0, s, bd.planes, p ? p->K : 0, stride, size_t(p ? p->K : 0) * stride, hd.a1, \
                                     hd.j1, nullptr, nullptr, d.own_count(), bd.list, bd.sched, g, d.own_pos(), d.vel, d.acc, hd.jerk, d.keep, d.escaped, bd.tau,  \
                                     bd.level, T, max_level, tick, abs_dt, eta, b, d.inter)
    if (p) HMFIN(true); else HMFIN(false);
#undef HMFIN
}

void launch_hm_act_reduce(hipStream_t s, const Dev& d, const HermiteDev& hd, const BlockDev& bd, const HmActPlan& p, int n_act, double g) {
    if (n_act <= 0) return;
    const size_t stride = size_t(p.groups) * 64;
    hipLaunchKernelGGL((k_hmb_finish<true, false>), dim3(blocks_for(n_act, 256)), dim3(256), 0, s, bd.planes, p.K, stride, size_t(p.K) * stride, nullptr,
                       nullptr, hd.a1, hd.j1, d.own_count(), bd.list, bd.sched, g, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0,
                       0.0, 0.0, 0.0, Bounds64{}, nullptr);
}

}  // namespace nbody64
