// kernels_pairs.hip -- the binary census of a handle's bodies on the device (gfx950), f64 on either dtype: nbody_partners and
// nbody_bound_pairs (include/nbody_hip.h, "binary census"), and the sticky mergers built on the same all-pairs frame:
// nbody_nearest, nbody_contacts and nbody_merge_contacts ("sticky mergers").  Compiled with -ffp-contract=off (every product,
// sum and difference rounded on its own; sqrt and divide are IEEE).  No floating-point atomics: the same input gives the same
// bits.  Every kernel is read-only but k_contact_emit<F, true>.
//
//   k_partner        the all-pairs pass.  One body per lane (position, velocity and mass in registers as doubles), the partners
//                    of a slice staged through LDS in tiles of 256 as k_hm_strict stages its own, j ascending, the best pair
//                    replaced on e < best only; the grid is (groups of 256 bodies) x K slices, one {energy, index} record per
//                    (slice, body).  kDist: the metric is the squared distance instead of the pair energy ("k_nearest") --
//                    positions only, no velocity tile, no sqrt, no divide
//   k_partner_merge  the K records of a body in slice order under the same strict <: the lowest j among equal energies,
//                    whatever K is
//   k_pair_flag      1 where partner[partner[i]] == i, e < 0 and i < partner[i]
//   (rocprim::exclusive_scan over the integer flags: integer addition is associative, its order cannot show)
//   k_pair_emit      the orbital elements of the flagged pairs into their slot of the list
//   k_contact_flag   1 where nearest[nearest[i]] == i, r2 < R2 and i < nearest[i]
//   k_contact_emit   the NbodyContact of the flagged pairs into their slot; kApply: the merged record into row i, the keep
//                    flags of every live row for the retain that follows (k_compact / k_hm_compact), and *escaped raised
#include "kernels_pairs.h"
#include "kernels.h"   // nbody::tuning()
#include "pair_tiles.h"
#include "real.h"      // widen
#include "scratch_carve.h"

#include <rocprim/device/device_scan.hpp>

#include <algorithm>

namespace nbody {

using pairs::kPairBlock;

namespace {

// e_ij = 0.5 w2 - (g (m_i + m_j)) / sqrt(r2): d and w change sign with i <-> j, their squares do not, and the sum of the masses
// commutes -- e_ij == e_ji bit for bit
__device__ __forceinline__ double pair_energy(const double4 pi, const double4 vi, const double4 pj, const double4 vj, double g, double soft2) {
    const double dx = pj.x - pi.x, dy = pj.y - pi.y, dz = pj.z - pi.z;
    const double wx = vj.x - vi.x, wy = vj.y - vi.y, wz = vj.z - vi.z;
    const double r2 = ((dx * dx + dy * dy) + dz * dz) + soft2;
    const double w2 = (wx * wx + wy * wy) + wz * wz;
    return 0.5 * w2 - (g * (pi.w + pj.w)) / __builtin_sqrt(r2);
}

// r2_ij = (dx dx + dy dy) + dz dz, unsoftened: d changes sign with i <-> j, its squares do not -- r2_ij == r2_ji bit for bit
__device__ __forceinline__ double pair_dist2(const double4 pi, const double4 pj) {
    const double dx = pj.x - pi.x, dy = pj.y - pi.y, dz = pj.z - pi.z;
    return (dx * dx + dy * dy) + dz * dz;
}

}  // namespace

template <class F, bool kDist>
__global__ __launch_bounds__(kPairBlock) void k_partner(const typename Real<F>::V4* __restrict__ pos,
                                                        const typename Real<F>::V4* __restrict__ vel, const int* __restrict__ count,
                                                        int n_upper, int groups, int K, double g, double soft2,
                                                        double* __restrict__ rec_e, int* __restrict__ rec_j) {
    __shared__ double4 tx[kPairBlock], tv[kDist ? 1 : kPairBlock];
    const int n = live_count(count, n_upper);
    const pairs::PairFrame f(groups, K, n);
    const int i = f.first + int(threadIdx.x);
    const bool live = i < n;
    const double4 pi = live ? widen(pos[i]) : make_double4(0.0, 0.0, 0.0, 0.0);
    const double4 vi = live && !kDist ? widen(vel[i]) : make_double4(0.0, 0.0, 0.0, 0.0);
    double best = inf64();
    int best_j = -1;
    pairs::for_each_partner(
        f,
        [&](int slot, int j) {
            tx[slot] = widen(pos[j]);
            if constexpr (!kDist) tv[slot] = widen(vel[j]);
        },
        [&](int j, int t) {
            double e;
            if constexpr (kDist) e = pair_dist2(pi, tx[t]);
            else e = pair_energy(pi, vi, tx[t], tv[t], g, soft2);
            if (j != i && e < best) { best = e; best_j = j; }     // (a NaN never wins; the i == i pair is left out)
        });
    if (live) {
        const size_t row = size_t(f.slice) * (size_t(groups) * kPairBlock) + size_t(i);
        rec_e[row] = best;
        rec_j[row] = best_j;
    }
}

__global__ __launch_bounds__(kPairBlock) void k_partner_merge(const int* __restrict__ count, int n_upper, int K, size_t stride,
                                                              const double* __restrict__ rec_e, const int* __restrict__ rec_j,
                                                              int* __restrict__ partner, double* __restrict__ energy) {
    const int i = blockIdx.x * kPairBlock + threadIdx.x;
    if (i >= n_upper) return;
    double best = inf64();
    int best_j = -1;
    if (i < *count) {
        for (int s = 0; s < K; ++s) {   // slices in ascending order hold ascending j
            const double e = rec_e[size_t(s) * stride + size_t(i)];
            if (e < best) { best = e; best_j = rec_j[size_t(s) * stride + size_t(i)]; }
        }
    }
    partner[i] = best_j;
    energy[i] = best;
}

__global__ __launch_bounds__(kPairBlock) void k_pair_flag(const int* __restrict__ count, int n_upper, const int* __restrict__ partner,
                                                          const double* __restrict__ energy, int* __restrict__ flag) {
    const int i = blockIdx.x * kPairBlock + threadIdx.x;
    if (i >= n_upper) return;
    const int n = min(*count, n_upper);
    int f = 0;
    if (i < n) {
        const int j = partner[i];
        if (j > i && j < n && partner[j] == i && energy[i] < 0.0) f = 1;
    }
    flag[i] = f;
}

template <class F>
__global__ __launch_bounds__(kPairBlock) void k_pair_emit(const typename Real<F>::V4* __restrict__ pos,
                                                          const typename Real<F>::V4* __restrict__ vel, int n_upper, double g,
                                                          const int* __restrict__ partner, const double* __restrict__ energy,
                                                          const int* __restrict__ flag, const int* __restrict__ offset,
                                                          NbodyBoundPair* __restrict__ out, int* __restrict__ total) {
    const int i = blockIdx.x * kPairBlock + threadIdx.x;
    if (i >= n_upper) return;
    if (i == n_upper - 1) *total = offset[i] + flag[i];
    if (!flag[i]) return;
    const int j = partner[i];
    const double4 pi = widen(pos[i]), vi = widen(vel[i]), pj = widen(pos[j]), vj = widen(vel[j]);
    const double dx = pj.x - pi.x, dy = pj.y - pi.y, dz = pj.z - pi.z;
    const double wx = vj.x - vi.x, wy = vj.y - vi.y, wz = vj.z - vi.z;
    const double e = energy[i];
    const double M = pi.w + pj.w;
    const double gm = g * M;
    const double hx = dy * wz - dz * wy, hy = dz * wx - dx * wz, hz = dx * wy - dy * wx;
    const double h2 = (hx * hx + hy * hy) + hz * hz;
    const double a = gm / (-2.0 * e);
    const double q = 1.0 + ((2.0 * e) * h2) / (gm * gm);
    NbodyBoundPair r;
    r.i = i;
    r.j = j;
    r.energy = e;
    r.binding = ((pi.w * pj.w) / M) * e;
    r.semi_major = a;
    r.eccentricity = __builtin_sqrt(q > 0.0 ? q : 0.0);
    r.period = 6.283185307179586 * (a * __builtin_sqrt(a / gm));
    r.separation = __builtin_sqrt((dx * dx + dy * dy) + dz * dz);
    out[offset[i]] = r;   // (offset < pairs <= n_upper / 2: the first bodies of disjoint pairs)
}

__global__ __launch_bounds__(kPairBlock) void k_contact_flag(const int* __restrict__ count, int n_upper, const int* __restrict__ nearest,
                                                             const double* __restrict__ dist2, double R2, int* __restrict__ flag) {
    const int i = blockIdx.x * kPairBlock + threadIdx.x;
    if (i >= n_upper) return;
    const int n = min(*count, n_upper);
    int f = 0;
    if (i < n) {
        const int j = nearest[i];
        if (j > i && j < n && nearest[j] == i && dist2[i] < R2) f = 1;   // (strict: a pair at exactly R2 is no contact)
    }
    flag[i] = f;
}

namespace {
// q = ((m_i q_i) + (m_j q_j)) / M per component, every operation rounded on its own; M == 0: (q_i + q_j) 0.5
__device__ __forceinline__ double merged1(double mi, double qi, double mj, double qj, double M) {
    return M == 0.0 ? (qi + qj) * 0.5 : ((mi * qi) + (mj * qj)) / M;
}
template <class F>
__device__ __forceinline__ typename Real<F>::V4 merged4(double mi, const double4 qi, double mj, const double4 qj, double M, double w) {
    return Real<F>::make4(F(merged1(mi, qi.x, mj, qj.x, M)), F(merged1(mi, qi.y, mj, qj.y, M)), F(merged1(mi, qi.z, mj, qj.z, M)), F(w));
}
}  // namespace

// The pairs are disjoint and thread i handles pair (i, j) alone: rows i and j are read and written by nobody else.  kApply:
// every live row's keep byte has exactly one writer -- a body that is not the j of a flagged pair writes its own 1, the
// flagged i writes keep[j] = 0.  jerk: a Hermite handle's held j0 (else null), carried like the acceleration.
template <class F, bool kApply>
__global__ __launch_bounds__(kPairBlock) void k_contact_emit(typename Real<F>::V4* __restrict__ pos, typename Real<F>::V4* __restrict__ vel,
                                                             typename Real<F>::V4* __restrict__ acc, typename Real<F>::V4* __restrict__ jerk,
                                                             const int* __restrict__ count, int n_upper, const int* __restrict__ nearest,
                                                             const double* __restrict__ dist2, const int* __restrict__ flag,
                                                             const int* __restrict__ offset, NbodyContact* __restrict__ out,
                                                             int* __restrict__ total, unsigned char* __restrict__ keep,
                                                             int* __restrict__ escaped) {
    const int i = blockIdx.x * kPairBlock + threadIdx.x;
    if (i >= n_upper) return;
    if (i == n_upper - 1) *total = offset[i] + flag[i];
    if (!flag[i]) {
        if (kApply && i < min(*count, n_upper)) {
            const int p = nearest[i];
            const bool absorbed = p >= 0 && p < i && flag[p] && nearest[p] == i;
            if (!absorbed) keep[i] = 1;
        }
        return;
    }
    const int j = nearest[i];
    const double4 pi = widen(pos[i]), vi = widen(vel[i]), pj = widen(pos[j]), vj = widen(vel[j]);
    const double wx = vj.x - vi.x, wy = vj.y - vi.y, wz = vj.z - vi.z;
    const double w2 = (wx * wx + wy * wy) + wz * wz;
    const double mi = pi.w, mj = pj.w, M = mi + mj;
    NbodyContact r;
    r.i = i;
    r.j = j;
    r.into = 0;   // (the host fills it from the list)
    r.reserved = 0;
    r.separation = __builtin_sqrt(dist2[i]);
    r.mass = M;
    r.dkinetic = M == 0.0 ? 0.0 : -0.5 * (((mi * mj) / M) * w2);
    out[offset[i]] = r;   // (offset < contacts <= n_upper / 2: the first bodies of disjoint pairs)
    if (kApply) {
        const double4 ai = widen(acc[i]), aj = widen(acc[j]);
        pos[i] = merged4<F>(mi, pi, mj, pj, M, M);
        vel[i] = merged4<F>(mi, vi, mj, vj, M, 0.0);
        acc[i] = merged4<F>(mi, ai, mj, aj, M, 0.0);
        if (jerk) jerk[i] = merged4<F>(mi, widen(jerk[i]), mj, widen(jerk[j]), M, 0.0);
        keep[i] = 1;
        keep[j] = 0;
        atomicAdd(escaped, 1);   // (an integer: the retain looks only at != 0)
    }
}

namespace pairs {

PartnerPlan make_partner_plan(int n_upper) { return make_partner_plan(n_upper, n_upper); }

PartnerPlan make_partner_plan(int n_upper, int partners) {
    PartnerPlan p;
    const int want = nbody::tuning().bf64_waves > 0 ? nbody::tuning().bf64_waves : 2048;
    p.groups = blocks_for(n_upper);
    const int waves = p.groups * (kPairBlock / 64);
    p.K = std::max(1, std::min(want / std::max(1, waves), (partners + 63) / 64));   // (a slice holds 64 partners or more)
    return p;
}

size_t scan_tmp_bytes(size_t n) {
    size_t b = 0;
    int* v = nullptr;
    (void)rocprim::exclusive_scan(nullptr, b, v, v, 0, n, rocprim::plus<int>(), 0);
    return b;
}

namespace {
PairScratch layout(Carver& c, size_t n_upper, const PartnerPlan& p, bool want_pairs) {
    const size_t rows = size_t(p.K) * size_t(p.groups) * kPairBlock;
    PairScratch w;
    w.rec_e = c.take<double>(rows);
    w.rec_j = c.take<int>(rows);
    w.energy = c.take<double>(n_upper);
    w.partner = c.take<int>(n_upper);
    if (want_pairs) {
        w.flag = c.take<int>(n_upper);
        w.offset = c.take<int>(n_upper);
        w.total = c.take<int>(1);
        static_assert(sizeof(NbodyContact) <= sizeof(NbodyBoundPair), "the list block is sized for the larger record");
        w.pairs = c.take<NbodyBoundPair>(n_upper / 2 + 1);
        w.contacts = reinterpret_cast<NbodyContact*>(w.pairs);   // (a call lists one kind)
        w.scan_bytes = scan_tmp_bytes(n_upper);
        w.scan_tmp = c.take<char>(w.scan_bytes);
    }
    return w;
}
}  // namespace

size_t scratch_bytes(size_t n_upper, const PartnerPlan& p, bool want_pairs) { Carver c; layout(c, n_upper, p, want_pairs); return c.offset(); }
PairScratch scratch_layout(void* base, size_t n_upper, const PartnerPlan& p, bool want_pairs) {
    Carver c(base);
    return layout(c, n_upper, p, want_pairs);
}

template <class F>
void launch_partners(hipStream_t s, const ShardT<F>& sh, int n_upper, const PartnerPlan& p, double g, double soft2, const PairScratch& w) {
    if (n_upper <= 0 || p.groups <= 0) return;
    hipLaunchKernelGGL((k_partner<F, false>), dim3(unsigned(p.groups) * unsigned(p.K)), dim3(kPairBlock), 0, s, sh.own_pos(), sh.vel,
                       sh.own_count(), n_upper, p.groups, p.K, g, soft2, w.rec_e, w.rec_j);
    hipLaunchKernelGGL(k_partner_merge, dim3(blocks_for(n_upper)), dim3(kPairBlock), 0, s, sh.own_count(), n_upper, p.K,
                       size_t(p.groups) * kPairBlock, w.rec_e, w.rec_j, w.partner, w.energy);
}

template <class F>
void launch_nearest(hipStream_t s, const ShardT<F>& sh, int n_upper, const PartnerPlan& p, const PairScratch& w) {
    if (n_upper <= 0 || p.groups <= 0) return;
    hipLaunchKernelGGL((k_partner<F, true>), dim3(unsigned(p.groups) * unsigned(p.K)), dim3(kPairBlock), 0, s, sh.own_pos(), sh.vel,
                       sh.own_count(), n_upper, p.groups, p.K, 0.0, 0.0, w.rec_e, w.rec_j);
    hipLaunchKernelGGL(k_partner_merge, dim3(blocks_for(n_upper)), dim3(kPairBlock), 0, s, sh.own_count(), n_upper, p.K,
                       size_t(p.groups) * kPairBlock, w.rec_e, w.rec_j, w.partner, w.energy);
}

template <class F>
int launch_bound_pairs(hipStream_t s, const ShardT<F>& sh, int n_upper, double g, const PairScratch& w) {
    if (n_upper <= 0) return 0;
    const int blocks = blocks_for(n_upper);
    hipLaunchKernelGGL(k_pair_flag, dim3(blocks), dim3(kPairBlock), 0, s, sh.own_count(), n_upper, w.partner, w.energy, w.flag);
    size_t tb = w.scan_bytes;
    if (rocprim::exclusive_scan(w.scan_tmp, tb, w.flag, w.offset, 0, size_t(n_upper), rocprim::plus<int>(), s) != hipSuccess) return -1;
    hipLaunchKernelGGL(k_pair_emit<F>, dim3(blocks), dim3(kPairBlock), 0, s, sh.own_pos(), sh.vel, n_upper, g, w.partner, w.energy, w.flag,
                       w.offset, w.pairs, w.total);
    return 0;
}

template <class F>
int launch_contacts(hipStream_t s, const ShardT<F>& sh, int n_upper, double R2, const PairScratch& w) {
    if (n_upper <= 0) return 0;
    const int blocks = blocks_for(n_upper);
    hipLaunchKernelGGL(k_contact_flag, dim3(blocks), dim3(kPairBlock), 0, s, sh.own_count(), n_upper, w.partner, w.energy, R2, w.flag);
    size_t tb = w.scan_bytes;
    if (rocprim::exclusive_scan(w.scan_tmp, tb, w.flag, w.offset, 0, size_t(n_upper), rocprim::plus<int>(), s) != hipSuccess) return -1;
    hipLaunchKernelGGL((k_contact_emit<F, false>), dim3(blocks), dim3(kPairBlock), 0, s, sh.own_pos(), sh.vel, sh.acc,
                       static_cast<typename ShardT<F>::V4*>(nullptr), sh.own_count(), n_upper, w.partner, w.energy, w.flag, w.offset,
                       w.contacts, w.total, sh.keep, sh.escaped);
    return 0;
}

template <class F>
void launch_merge(hipStream_t s, const ShardT<F>& sh, typename ShardT<F>::V4* jerk, int n_upper, const PairScratch& w) {
    if (n_upper <= 0) return;
    hipLaunchKernelGGL((k_contact_emit<F, true>), dim3(blocks_for(n_upper)), dim3(kPairBlock), 0, s, sh.own_pos(), sh.vel, sh.acc, jerk,
                       sh.own_count(), n_upper, w.partner, w.energy, w.flag, w.offset, w.contacts, w.total, sh.keep, sh.escaped);
}

template void launch_nearest<float>(hipStream_t, const ShardT<float>&, int, const PartnerPlan&, const PairScratch&);
template void launch_nearest<double>(hipStream_t, const ShardT<double>&, int, const PartnerPlan&, const PairScratch&);
template int launch_contacts<float>(hipStream_t, const ShardT<float>&, int, double, const PairScratch&);
template int launch_contacts<double>(hipStream_t, const ShardT<double>&, int, double, const PairScratch&);
template void launch_merge<float>(hipStream_t, const ShardT<float>&, float4*, int, const PairScratch&);
template void launch_merge<double>(hipStream_t, const ShardT<double>&, double4*, int, const PairScratch&);
template void launch_partners<float>(hipStream_t, const ShardT<float>&, int, const PartnerPlan&, double, double, const PairScratch&);
template void launch_partners<double>(hipStream_t, const ShardT<double>&, int, const PartnerPlan&, double, double, const PairScratch&);
template int launch_bound_pairs<float>(hipStream_t, const ShardT<float>&, int, double, const PairScratch&);
template int launch_bound_pairs<double>(hipStream_t, const ShardT<double>&, int, double, const PairScratch&);

}}  // namespace nbody::pairs
