// kernels_bf64.hip -- fast all-pairs gravity for F = f64 handles (NBODY_MATH_FAST on a brute-force NBODY_F64 handle):
// the f32 symmetric scheme of kernels_bf_sym.hip restated for double4 state.  Each unordered pair is evaluated once and
// applied to both bodies, as BruteForceSimulation::update_forces does on the CPU (brute_force.rs:70-81).
//
//   k_bf64_sym      a wave keeps a RESIDENT SET of 64*IPT bodies in registers; TRAVELLING CHUNKS of 64 bodies, each with
//                   its own accumulators, pass through the lanes one lane per step.  Set a meets the chunks of sets
//                   a+1 .. a+ceil(A/2)-1 (cyclic); a set's chunk sequence is cut into K slices, one per wave.
//                   ROT = 0: the chunk's positions sit in the wave's own LDS tile and lane l reads the one it meets
//                   (ds_read_b128 x2); only the three accumulators travel through the crossbar (6 ds_bpermute_b32 per
//                   step).  ROT = 1: positions travel too (14 ds_bpermute_b32 per step, as the f32 kernel does).
//   k_bf64_os       one-sided, one body per lane, partners staged 64 at a time in the wave's LDS tile and read back as
//                   wave-uniform broadcasts.  MODE 0: every own body (small worlds, where k_bf64_sym cannot fill the
//                   chip); MODE 1: the pairs k_bf64_sym leaves over (the own set and, for even A, the opposite set);
//                   MODE 2: the bodies of the other index blocks (sharded worlds).  The partner list is cut into K slices.
//   k_bf64_reduce   the planes added in a fixed order (bit-reproducible), times g; KICK fuses integrate_after_force in
//                   k_kick_drift's arithmetic.
//
// Pair arithmetic: rinv = rsqrt(r2 + eps2) (ocml: v_rsq_f64 and a Newton step), rinv^3, one product per side and three
// explicit FMAs per side (the library builds with -ffp-contract=off).  Every plane entry is written exactly once per
// launch; there are no atomics on the planes.
#include "kernels_f64.h"
#include "kernels.h"   // nbody::tuning()
#include "pair64.h"
#include "partner_stream.h"   // Win, n_windows, window

namespace nbody64 {

namespace {

using namespace pair64;   // kPad, pad_body, rot64, plane_sum
using nbody::Win;
using nbody::n_windows;
using nbody::window;

// IPT unordered pairs (resident q, traveller j), written stage by stage so that no instruction waits on its predecessor
template <int IPT>
__device__ __forceinline__ void pair_evals64(const double (&xi)[IPT], const double (&yi)[IPT], const double (&zi)[IPT], const double (&mi)[IPT],
                                             double (&axi)[IPT], double (&ayi)[IPT], double (&azi)[IPT], double xj, double yj, double zj,
                                             double mj, double& axj, double& ayj, double& azj, double eps2) {
    // four at a time: the stage temporaries of eight would push the IPT = 8 kernel past the register file
#pragma unroll
    for (int q0 = 0; q0 < IPT; q0 += 4) {
        constexpr int B = IPT < 4 ? IPT : 4;
        double dx[B], dy[B], dz[B], r[B], sj[B];
#pragma unroll
        for (int u = 0; u < B; ++u) { dx[u] = xj - xi[q0 + u]; dy[u] = yj - yi[q0 + u]; dz[u] = zj - zi[q0 + u]; }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < B; ++u) r[u] = fma(dx[u], dx[u], eps2);
#pragma unroll
        for (int u = 0; u < B; ++u) r[u] = fma(dy[u], dy[u], r[u]);
#pragma unroll
        for (int u = 0; u < B; ++u) r[u] = fma(dz[u], dz[u], r[u]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < B; ++u) r[u] = rsqrt(r[u]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < B; ++u) sj[u] = r[u] * r[u];
#pragma unroll
        for (int u = 0; u < B; ++u) r[u] = sj[u] * r[u];          // rinv^3
#pragma unroll
        for (int u = 0; u < B; ++u) sj[u] = mj * r[u];            // what body j does to body i
#pragma unroll
        for (int u = 0; u < B; ++u) r[u] = mi[q0 + u] * r[u];     // what body i does to body j
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < B; ++u) {
            axi[q0 + u] = fma(dx[u], sj[u], axi[q0 + u]);
            ayi[q0 + u] = fma(dy[u], sj[u], ayi[q0 + u]);
            azi[q0 + u] = fma(dz[u], sj[u], azi[q0 + u]);
            axj = fma(-dx[u], r[u], axj);
            ayj = fma(-dy[u], r[u], ayj);
            azj = fma(-dz[u], r[u], azj);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

// 4 waves per workgroup; wave gw = a * K + part is slice `part` of resident set a
template <int IPT, int ROT>
__global__ __launch_bounds__(256) void k_bf64_sym(const double4* __restrict__ pos, const int* __restrict__ count, int A, int K, int sym_sets,
                                                  double4* __restrict__ planes, size_t plane_stride, double eps2) {
    __shared__ double4 tile[ROT == 0 ? 4 : 1][64];
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
    // eps2 in a VGPR (see kernels_bf_sym.hip: an SGPR operand makes the compiler drain all LDS traffic every step)
    double eps2v = eps2;
    asm volatile("" : "+v"(eps2v));

    double xi[IPT], yi[IPT], zi[IPT], mi[IPT], axi[IPT], ayi[IPT], azi[IPT];
#pragma unroll
    for (int q = 0; q < IPT; ++q) {
        const int i = (a * IPT + q) * 64 + lane;
        const double4 p = (i < n) ? pos[i] : pad_body();
        xi[q] = p.x; yi[q] = p.y; zi[q] = p.z; mi[q] = p.w;
        axi[q] = ayi[q] = azi[q] = 0.0;
    }
    auto chunk_of = [&](int k) {
        int c = (a + 1) * IPT + k;
        if (c >= Cn) c -= Cn;
        return c;
    };
    auto load_chunk = [&](int k) {
        const int j = chunk_of(k) * 64 + lane;
        return (j < n) ? pos[j] : pad_body();
    };
    double4 nxt = (k0 < k1) ? load_chunk(k0) : pad_body();
    for (int k = k0; k < k1; ++k) {
        const double4 cur = nxt;
        if (k + 1 < k1) nxt = load_chunk(k + 1);
        double axj = 0.0, ayj = 0.0, azj = 0.0;
        // at step s lane l meets the body that started in lane (l - s) & 63, whose accumulators it holds
        if (ROT == 0) {
            tile[wv][lane] = cur;   // the wave's own tile: its LDS operations complete in program order
            for (int s = 0; s < 64; ++s) {
                const double4 pj = tile[wv][(lane - s) & 63];
                pair_evals64<IPT>(xi, yi, zi, mi, axi, ayi, azi, pj.x, pj.y, pj.z, pj.w, axj, ayj, azj, eps2v);
                axj = rot64(axj, src1); ayj = rot64(ayj, src1); azj = rot64(azj, src1);
            }
        } else {
            double xj = cur.x, yj = cur.y, zj = cur.z, mj = cur.w;
            for (int s = 0; s < 64; ++s) {
                // the next step's position is requested before this step's arithmetic: the crossbar latency hides behind it
                const double x1 = rot64(xj, src1), y1 = rot64(yj, src1), z1 = rot64(zj, src1), m1 = rot64(mj, src1);
                pair_evals64<IPT>(xi, yi, zi, mi, axi, ayi, azi, xj, yj, zj, mj, axj, ayj, azj, eps2v);
                axj = rot64(axj, src1); ayj = rot64(ayj, src1); azj = rot64(azj, src1);
                xj = x1; yj = y1; zj = z1; mj = m1;
            }
        }
        const int d = k / IPT + 1;   // set distance 1..sym_sets
        planes[size_t(d - 1) * plane_stride + size_t(chunk_of(k)) * 64 + lane] = make_double4(axj, ayj, azj, 0.0);
    }
    double4* __restrict__ out = planes + size_t(sym_sets + part) * plane_stride;
#pragma unroll
    for (int q = 0; q < IPT; ++q) out[size_t(a * IPT + q) * 64 + lane] = make_double4(axi[q], ayi[q], azi[q], 0.0);
}

// 4 waves per workgroup; wave gw = group * K + slice: bodies group*64 + lane of the own block against slice `slice` of
// the partner list.  Output: plane `slice`, rows group*64 .. group*64+63 (every row, padding included).
template <int MODE>
__global__ __launch_bounds__(256) void k_bf64_os(const double4* __restrict__ pos_all, const int* __restrict__ seg_count, int n_seg,
                                                 int seg_cap, int my_seg, int set_size, int A, int groups, int K,
                                                 double4* __restrict__ planes, size_t plane_stride, double eps2) {
    __shared__ double4 tile[4][64];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int gw = blockIdx.x * 4 + wv;
    if (gw >= groups * K) return;
    const int group = gw / K, slice = gw - group * K;
    const int n_own = seg_count[my_seg];
    const int i = group * 64 + lane;
    const double4 pi = (i < n_own) ? pos_all[size_t(my_seg) * seg_cap + i] : pad_body();
    const int a = (group * 64) / set_size;       // (MODE 1: the set of all 64 bodies of the group)
    double eps2v = eps2;
    asm volatile("" : "+v"(eps2v));
    const int nw = n_windows<MODE>(n_seg, A);
    long long R = 0;
    for (int w = 0; w < nw; ++w) {
        const Win win = window<MODE>(w, seg_count, my_seg, n_own, set_size, A, a);
        R += max(0, win.hi - win.lo);
    }
    const long long r0 = R * slice / K, r1 = R * (slice + 1) / K;
    double ax = 0.0, ay = 0.0, az = 0.0;
    long long first = 0;   // index of the window's first body in the concatenated partner list
    for (int w = 0; w < nw; ++w) {
        const Win win = window<MODE>(w, seg_count, my_seg, n_own, set_size, A, a);
        const int len = max(0, win.hi - win.lo);
        const long long lo = max(r0, first), hi = min(r1, first + len);
        if (lo < hi) {
            const double4* __restrict__ ps = pos_all + size_t(win.seg) * seg_cap + win.lo;   // ps[c - first]: partner c
            // the own body's place in the concatenated list (never met when the window is another segment's)
            const long long self = (win.seg == my_seg && i >= win.lo && i < win.hi) ? first + (i - win.lo) : -1;
            double4 nxt = (lo + lane < hi) ? ps[lo + lane - first] : pad_body();
            for (long long c0 = lo; c0 < hi; c0 += 64) {
                tile[wv][lane] = nxt;   // the wave's own tile: its LDS operations complete in program order
                if (c0 + 64 + lane < hi) nxt = ps[c0 + 64 + lane - first];
                const int cnt = int(min(64LL, hi - c0));
                for (int t = 0; t < cnt; ++t) {
                    const double4 pj = tile[wv][t];   // wave-uniform address: an LDS broadcast
                    const double dx = pj.x - pi.x, dy = pj.y - pi.y, dz = pj.z - pi.z;
                    const double r2 = fma(dz, dz, fma(dy, dy, fma(dx, dx, eps2v)));
                    const double rinv = rsqrt(r2);
                    double sj = pj.w * ((rinv * rinv) * rinv);
                    sj = (c0 + t == self) ? 0.0 : sj;   // the reference never forms the i == j pair (brute_force.rs:70-71)
                    ax = fma(dx, sj, ax);
                    ay = fma(dy, sj, ay);
                    az = fma(dz, sj, az);
                }
            }
        }
        first += len;
    }
    planes[size_t(slice) * plane_stride + i] = make_double4(ax, ay, az, 0.0);
}

// the planes added in a fixed order, times g; KICK: integrate_after_force (shared.rs:141-148) in k_kick_drift's arithmetic
template <bool KICK>
__global__ __launch_bounds__(256) void k_bf64_reduce(const double4* __restrict__ planes, int n_planes, size_t plane_stride,
                                                     const int* __restrict__ count, double g, double4* __restrict__ acc,
                                                     double4* __restrict__ pos, double4* __restrict__ vel, double dt,
                                                     const int* __restrict__ seg_count, int n_seg, unsigned long long* __restrict__ inter) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (inter && i == 0) {   // NbodyStats::interactions of this force pass, from the live counts
        long long tot = 0;
        for (int s = 0; s < n_seg; ++s) tot += seg_count[s];
        if (tot > 0) atomicAdd(inter, (unsigned long long)(*count) * (unsigned long long)(tot - 1));
    }
    if (i >= *count) return;
    double4 a, no_j;
    plane_sum<1>(planes, n_planes, plane_stride, 0, i, g, a, no_j);
    acc[i] = a;
    if (KICK) {
        double4 p = pos[i], v = vel[i];
        v.x += a.x * dt;
        v.y += a.y * dt;
        v.z += a.z * dt;
        p.x += (v.x * 0.5) * dt;
        p.y += (v.y * 0.5) * dt;
        p.z += (v.z * 0.5) * dt;
        vel[i] = v;
        pos[i] = p;
    }
}

inline int blocks4(long long waves) { return int((waves + 3) / 4); }

}  // namespace

// ----------------------------------------------------------------------------------- host side
Bf64Plan make_bf64_plan(int n_upper, int n_remote_upper, int n_seg, int force_ipt) {
    const nbody::Tuning& t = nbody::tuning();
    Bf64Plan p;
    const int n = n_upper > 0 ? n_upper : 1;
    p.groups = (n + 63) / 64;
    p.sym = n >= std::max(2, t.bf64_min_bodies);
    if (p.sym) {
        p.ipt = force_ipt ? force_ipt : t.bf64_ipt == 4 || t.bf64_ipt == 8 ? t.bf64_ipt : (n <= kBf64SmallIptBelow ? 4 : 8);
        p.rot = t.bf64_rot == 1 ? 1 : 0;
        p.A = (n + 64 * p.ipt - 1) / (64 * p.ipt);
        p.sym_sets = (p.A + 1) / 2 - 1;
        const int L = p.ipt * p.sym_sets;
        const int want = t.bf64_waves > 0 ? t.bf64_waves : 2048;
        p.K = p.sym_sets > 0 ? std::max(1, std::min(L, (want + p.A - 1) / p.A)) : 0;
        p.groups = p.A * p.ipt;   // every 64-body group of the padded array
        p.k_own = std::max(1, std::min(16, (want + p.groups - 1) / p.groups));   // the left-over pairs (k_bf64_os MODE 1)
    } else {
        // every own pair one-sided, the partners cut into slices of at least 128 bodies
        const int want = t.bf64_waves > 0 ? t.bf64_waves : 2048;
        p.k_own = std::max(1, std::min((n + 127) / 128, (want + p.groups - 1) / p.groups));
    }
    p.n_pad = size_t(p.groups) * 64;
    if (n_seg > 1) {
        const int want = t.bf64_waves > 0 ? t.bf64_waves : 2048;
        p.k_remote = std::max(1, std::min(std::max(1, (n_remote_upper + 127) / 128), (want + p.groups - 1) / p.groups));
    }
    p.n_planes = p.sym_sets + p.K + p.k_own + p.k_remote;
    return p;
}

uint64_t bf64_sym_pairs(const Bf64Plan& p, size_t n) {
    if (!p.sym) return 0;
    const size_t set = size_t(64) * p.ipt;
    auto size_of = [&](int a) { size_t lo = size_t(a) * set; return lo >= n ? size_t(0) : std::min(set, n - lo); };
    uint64_t pairs = 0;
    for (int a = 0; a < p.A; ++a)
        for (int d = 1; d <= p.sym_sets; ++d) pairs += uint64_t(size_of(a)) * uint64_t(size_of((a + d) % p.A));
    return pairs;
}

void launch_bf64_sym(hipStream_t s, const Dev& d, const Bf64Plan& p, double4* planes, double eps2) {
    if (!p.sym || p.sym_sets <= 0) return;
    const dim3 grid(blocks4((long long)p.A * p.K)), block(256);
#define SYM64(I, R) hipLaunchKernelGGL((k_bf64_sym<I, R>), grid, block, 0, s, d.own_pos(), d.own_count(), p.A, p.K, p.sym_sets, planes, p.n_pad, eps2)
    if (p.ipt == 4) { if (p.rot) SYM64(4, 1); else SYM64(4, 0); }
    else { if (p.rot) SYM64(8, 1); else SYM64(8, 0); }
#undef SYM64
}

void launch_bf64_own(hipStream_t s, const Dev& d, const Bf64Plan& p, double4* planes, double eps2) {
    double4* out = planes + size_t(p.sym_sets + p.K) * p.n_pad;
    const dim3 grid(blocks4((long long)p.groups * p.k_own)), block(256);
    if (p.sym)
        hipLaunchKernelGGL(k_bf64_os<1>, grid, block, 0, s, d.pos_all, d.seg_count, d.n_seg, d.seg_cap, d.my_seg, 64 * p.ipt, p.A, p.groups, p.k_own,
                           out, p.n_pad, eps2);
    else
        hipLaunchKernelGGL(k_bf64_os<0>, grid, block, 0, s, d.pos_all, d.seg_count, d.n_seg, d.seg_cap, d.my_seg, 64, 1, p.groups, p.k_own,
                           out, p.n_pad, eps2);
}

void launch_bf64_remote(hipStream_t s, const Dev& d, const Bf64Plan& p, double4* planes, double eps2) {
    if (p.k_remote <= 0 || d.n_seg < 2) return;
    double4* out = planes + size_t(p.sym_sets + p.K + p.k_own) * p.n_pad;
    hipLaunchKernelGGL(k_bf64_os<2>, dim3(blocks4((long long)p.groups * p.k_remote)), dim3(256), 0, s, d.pos_all, d.seg_count, d.n_seg, d.seg_cap,
                       d.my_seg, 64, 1, p.groups, p.k_remote, out, p.n_pad, eps2);
}

void launch_bf64_reduce(hipStream_t s, const Dev& d, const Bf64Plan& p, const double4* planes, int n_upper, double g, const double* kick_dt) {
    if (n_upper <= 0) return;
    const dim3 grid((n_upper + 255) / 256), block(256);
    if (kick_dt)
        hipLaunchKernelGGL(k_bf64_reduce<true>, grid, block, 0, s, planes, p.n_planes, p.n_pad, d.own_count(), g, d.acc, d.own_pos(), d.vel, *kick_dt,
                           d.seg_count, d.n_seg, d.inter);
    else
        hipLaunchKernelGGL(k_bf64_reduce<false>, grid, block, 0, s, planes, p.n_planes, p.n_pad, d.own_count(), g, d.acc, d.own_pos(), d.vel, 0.0,
                           d.seg_count, d.n_seg, d.inter);
}

}  // namespace nbody64
