// sample_device.h -- the device code of the grid gathers, stated once, and the one dispatch of their launchers.  k_sample
// (kernels_sample.hip), k_pm_gather (kernels_pm.hip) and k_mesh_kick (kernels_mesh.hip) set a lane's stencil up with
// LaneStencil::set_up and form every component of the gradient with gradient_component<K>, so that a component of any of them is
// one fixed expression tree; the three kernels differ in what they store.  k_sample and k_mesh_kick take the three components
// from lane_gradient; k_pm_gather calls gradient_component itself, because its phi rides on the x component's loads.  k_sample's
// value and pregrad modes call weighted_sum; k_sample and k_pm_gather count the classes with count_classes.  The launchers pick
// the instance with for_reach_and_scheme.  The arithmetic is sample_grid.h's.  Device code only (hipcc, -ffp-contract=off).
#pragma once
#include "kernels_sample.h"
#include "device_util.h"   // live_count, wave_add

#include <type_traits>

namespace nbody { namespace sample {

// the linear index of a cell from its three indices on the grid (< 2^27: int arithmetic holds it)
__device__ __forceinline__ int cell_of(const deposit::Grid& g, int ix, int iy, int iz) { return (ix * g.dims[1] + iy) * g.dims[2] + iz; }

// What lane s of a gather holds of its point: the row (-1: none), the class (-1: no row), and the lane's copy of what the terms
// need, indexed by constants only.  rows: the rows in key order [n], or null: lane s takes row s.
template <int kCnt>
struct LaneStencil {
    int row, cls;
    bool active;                 // INSIDE or PARTIAL: the sums run
    long long f0, f1, f2;        // the stencil's first cell per axis
    double wx[3], wy[3], wz[3];
    int ix[kCnt], iy[kCnt], iz[kCnt];   // the stencil's indices on the grid, -1: the term is dropped

    __device__ __forceinline__ void set_up(const double* __restrict__ xyz, const int* __restrict__ count, int n, const deposit::Grid& g, int reach,
                                           const int* __restrict__ rows, int s) {
        const int live = count ? live_count(count, n) : n;
        row = -1;
        if (s < n) {
            const int r = rows ? rows[s] : s;   // (a permutation of 0 .. n - 1)
            if (r >= 0 && r < live) row = r;
        }
        // (a lane without a row takes the stencil of the grid's corner and drops it: the stencil is then written on every path)
        const double x = row >= 0 ? xyz[3 * size_t(row)] : g.origin[0], y = row >= 0 ? xyz[3 * size_t(row) + 1] : g.origin[1],
                     z = row >= 0 ? xyz[3 * size_t(row) + 2] : g.origin[2];
        deposit::Stencil st;
        const bool taken = deposit::body_stencil(g, x, y, z, 0.0, &st);
        cls = row < 0 ? -1 : taken ? sample::point_class(g, st, reach) : int(deposit::kSkipped);
        active = cls == deposit::kInside || cls == deposit::kPartial;
        f0 = f1 = f2 = 0;
#pragma unroll
        for (int t = 0; t < 3; ++t) wx[t] = wy[t] = wz[t] = 0.0;
        if (active) {
            f0 = st.first[0]; f1 = st.first[1]; f2 = st.first[2];
#pragma unroll
            for (int t = 0; t < 3; ++t) { wx[t] = st.w[0][t]; wy[t] = st.w[1][t]; wz[t] = st.w[2][t]; }
        }
        // the cells an axis has (uniform): kCnt on an axis in use, one on the ignored axis
        const int ca = g.axis == 0 ? 1 : kCnt, cb = g.axis == 1 ? 1 : kCnt, cc = g.axis == 2 ? 1 : kCnt;
#pragma unroll
        for (int t = 0; t < kCnt; ++t) {
            ix[t] = active && t < ca ? int(deposit::cell_on_axis(f0 + t, g.dims[0], g.periodic)) : -1;
            iy[t] = active && t < cb ? int(deposit::cell_on_axis(f1 + t, g.dims[1], g.periodic)) : -1;
            iz[t] = active && t < cc ? int(deposit::cell_on_axis(f2 + t, g.dims[2], g.periodic)) : -1;
        }
    }
};

// the sum of w G[cell] over the stencil in sample_grid.h's order; an index of -1 drops the term
template <int kCnt>
__device__ __forceinline__ double weighted_sum(const deposit::Grid& g, const double* __restrict__ G, const int (&ix)[kCnt], const int (&iy)[kCnt],
                                               const int (&iz)[kCnt], const double (&wx)[3], const double (&wy)[3], const double (&wz)[3],
                                               unsigned long long& reads) {
    double v[kCnt][kCnt][kCnt];
#pragma unroll
    for (int a = 0; a < kCnt; ++a)
#pragma unroll
        for (int b = 0; b < kCnt; ++b)
#pragma unroll
            for (int c = 0; c < kCnt; ++c) {
                const bool ok = ix[a] >= 0 && iy[b] >= 0 && iz[c] >= 0;
                v[a][b][c] = ok ? G[cell_of(g, ix[a], iy[b], iz[c])] : 0.0;
                reads += ok;
            }
    double sum = 0.0;
#pragma unroll
    for (int a = 0; a < kCnt; ++a)
#pragma unroll
        for (int b = 0; b < kCnt; ++b)
#pragma unroll
            for (int c = 0; c < kCnt; ++c)
                if (ix[a] >= 0 && iy[b] >= 0 && iz[c] >= 0) sum = sum + ((wx[a] * wy[b]) * wz[c]) * v[a][b][c];
    return sum;
}

// component K of the gradient, the differences formed on the fly: the kCnt + 2 kReach cells along axis K from the stencil's
// first cell - kReach on are read once for each of the other two axes' stencil cells.  kWithValue (K == 0, kCnt > 1, axis 0 in
// use): the middle kCnt planes are the stencil's own cells, read already, and *value becomes weighted_sum's sum over them -- the
// same terms in the same order -- with no further read.
template <int K, int kCnt, int kReach, bool kWithValue = false>
__device__ __forceinline__ double gradient_component(const deposit::Grid& g, const double* __restrict__ G, const LaneStencil<kCnt>& lane, double den,
                                                     unsigned long long& reads, double* value = nullptr) {
    static_assert(!kWithValue || (K == 0 && kCnt > 1), "the stencil's own cells are planes of the x component, and NGP reads none of them");
    const auto &ix = lane.ix, &iy = lane.iy, &iz = lane.iz;
    const auto &wx = lane.wx, &wy = lane.wy, &wz = lane.wz;
    const long long first_k = K == 0 ? lane.f0 : K == 1 ? lane.f1 : lane.f2;
    constexpr int kExt = kCnt + 2 * kReach;
    int e[kExt];
#pragma unroll
    for (int j = 0; j < kExt; ++j) e[j] = lane.active ? int(deposit::cell_on_axis(first_k - kReach + j, g.dims[K], g.periodic)) : -1;
    double v[kExt][kCnt][kCnt];   // [along K][the lower of the other two axes][the higher]
#pragma unroll
    for (int j = 0; j < kExt; ++j)
#pragma unroll
        for (int p = 0; p < kCnt; ++p)
#pragma unroll
            for (int q = 0; q < kCnt; ++q) {
                v[j][p][q] = 0.0;
                if (kCnt == 1 && j == kReach) continue;   // NGP: no difference reads its own cell
                const int cx = K == 0 ? e[j] : ix[p], cy = K == 1 ? e[j] : K == 0 ? iy[p] : iy[q], cz = K == 2 ? e[j] : iz[q];
                const bool ok = cx >= 0 && cy >= 0 && cz >= 0;
                if (ok) v[j][p][q] = G[cell_of(g, cx, cy, cz)];
                reads += ok;
            }
    if constexpr (kWithValue) {
        double s = 0.0;
#pragma unroll
        for (int a = 0; a < kCnt; ++a)
#pragma unroll
            for (int b = 0; b < kCnt; ++b)
#pragma unroll
                for (int c = 0; c < kCnt; ++c)
                    if (ix[a] >= 0 && iy[b] >= 0 && iz[c] >= 0) s = s + ((wx[a] * wy[b]) * wz[c]) * v[a + kReach][b][c];
        *value = s;
    }
    double sum = 0.0;
#pragma unroll
    for (int a = 0; a < kCnt; ++a)
#pragma unroll
        for (int b = 0; b < kCnt; ++b)
#pragma unroll
            for (int c = 0; c < kCnt; ++c) {
                const int t = K == 0 ? a : K == 1 ? b : c, p = K == 0 ? b : a, q = K == 2 ? b : c;
                bool ok = ix[a] >= 0 && iy[b] >= 0 && iz[c] >= 0 && e[t + kReach - 1] >= 0 && e[t + kReach + 1] >= 0;
                double d;
                if constexpr (kReach == 1) {
                    d = sample::diff2(v[t][p][q], v[t + 2][p][q], den);
                } else {
                    ok = ok && e[t] >= 0 && e[t + 4] >= 0;
                    d = sample::diff4(v[t][p][q], v[t + 1][p][q], v[t + 3][p][q], v[t + 4][p][q], den);
                }
                if (ok) sum = sum + ((wx[a] * wy[b]) * wz[c]) * d;
            }
    return sum;
}

// The gradient at a lane's point, component by component; the component along the ignored axis is +0.0 and reads nothing.
// (The sums are locals and reach grad at the end: stores through the reference between the components cost registers.)
template <int kCnt, int kReach>
__device__ __forceinline__ void lane_gradient(const deposit::Grid& g, const double* G, const LaneStencil<kCnt>& lane, double den,
                                              unsigned long long& reads, double (&grad)[3]) {
    const double gx = g.axis != 0 ? gradient_component<0, kCnt, kReach>(g, G, lane, den, reads) : 0.0;
    const double gy = g.axis != 1 ? gradient_component<1, kCnt, kReach>(g, G, lane, den, reads) : 0.0;
    const double gz = g.axis != 2 ? gradient_component<2, kCnt, kReach>(g, G, lane, den, reads) : 0.0;
    grad[0] = gx, grad[1] = gy, grad[2] = gz;
}

// The instance of a gather for a gradient operator and a grid's scheme: fn(reach, scheme) with the two as
// std::integral_constant<int, .>, so that kernel<decltype(reach)::value, decltype(scheme)::value> names it.  The one place
// where NBODY_SAMPLE_GRADIENT2 | 4 and NBODY_DEPOSIT_NGP | CIC | TSC become template arguments.
template <class Fn>
void for_scheme(int scheme, Fn&& fn) {   // (the scheme alone: k_sample's value and pregrad modes have no instance per reach)
    if (scheme == NBODY_DEPOSIT_NGP) fn(std::integral_constant<int, 0>());
    else if (scheme == NBODY_DEPOSIT_CIC) fn(std::integral_constant<int, 1>());
    else fn(std::integral_constant<int, 2>());
}
template <class Fn>
void for_reach_and_scheme(int gradient_op, int scheme, Fn&& fn) {
    if (gradient_op == NBODY_SAMPLE_GRADIENT2) for_scheme(scheme, [&](auto sc) { fn(std::integral_constant<int, 1>(), sc); });
    else for_scheme(scheme, [&](auto sc) { fn(std::integral_constant<int, 2>(), sc); });
}

// ix with the stencil cells dropped whose difference along the axis (first, dim) reads off the grid
template <int kCnt>
__device__ __forceinline__ void drop_unreached(const int (&ix)[kCnt], long long first, int dim, int periodic, int reach, int (&kept)[kCnt]) {
#pragma unroll
    for (int t = 0; t < kCnt; ++t) kept[t] = periodic || (first + t - reach >= 0 && first + t + reach < (long long)dim) ? ix[t] : -1;
}

// the four counts of a block's classes and its reads into the call's words: ballots and one integer atomic per wave and class
// (every lane of the wave is here)
__device__ __forceinline__ void count_classes(int cls, unsigned long long reads, Words* words) {
    unsigned long long n_of[4];
    for (int k = 0; k < 4; ++k) n_of[k] = (unsigned long long)__popcll(__ballot(cls == k));
    if (threadIdx.x % 64 == 0)
        for (int k = 0; k < 4; ++k)
            if (n_of[k]) atomicAdd(&words->counts[k], n_of[k]);
    wave_add(reads, &words->reads);
}

}}  // namespace nbody::sample
