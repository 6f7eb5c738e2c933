// kernels_sample.hip -- nbody_grid_sample and nbody_grid_sample_at on the device (gfx950): a grid read back at points with the
// deposit's NGP / CIC / TSC stencil, values and central-difference gradients (include/nbody_hip.h, "grid sample").  Compiled
// with -ffp-contract=off; the arithmetic is sample_grid.h's.  A gather: every lane reads the grid and writes its own row, so
// nothing depends on the order of the points.  No floating-point atomics, no LDS, no lane ever waits for another.  Every kernel
// reads the handle's state and writes the call's scratch only.
//
//   k_sample_stage  xyz[i] = the position of live row i, widened (the bodies; the caller's points are uploaded instead)
//   k_sample_keys   key[i] = the home cell of point i (rows past the live count and skipped points: `cells`, last), row[i] = i
//   (rocprim::radix_sort_pairs, stable, on (key, row): the points cell after cell, as kernels_deposit.hip orders the bodies)
//   k_grid_diff     sample_pregrad: D_k[c] for every cell c and k = 0, 1, 2 (+0.0 where the difference reads off the grid or k
//                   is the ignored axis: k_sample drops those terms by their indices and never reads the value)
//   k_sample        one lane per place of that order (or per row, unsorted), one instance per op and scheme.  The stencil's
//                   offsets are unrolled, so every index into the lane's arrays is a constant and they stay in registers; the
//                   loads of a sum are issued together, the sum follows in sample_grid.h's order.  In the gradient ops a
//                   component's stencil cells share their reads along the differentiated axis: cnt + 2 reach cells there, not
//                   2 reach cnt.  The counts come from ballots and one integer atomic per wave and class.
#include "kernels_sample.h"
#include "device_util.h"   // live_count, wave_add
#include "kernels.h"   // tuning()
#include "real.h"      // widen
#include "scratch_carve.h"

#include <rocprim/device/device_radix_sort.hpp>

namespace nbody {

using sample::kSampleBlock;

namespace {

enum { kModeValue = 0, kModeGrad2 = 1, kModeGrad4 = 2, kModePre = 3 };

// the linear index of a cell from its three indices on the grid (< 2^27: int arithmetic holds it)
__device__ __forceinline__ int cell_of(const deposit::Grid& g, int ix, int iy, int iz) { return (ix * g.dims[1] + iy) * g.dims[2] + iz; }

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

// component K of the gradient, the differences formed on the fly: the kCnt + 2 kReach cells along axis K from first_k - kReach
// on are read once for each of the other two axes' stencil cells
template <int K, int kCnt, int kReach>
__device__ __forceinline__ double gradient_component(const deposit::Grid& g, const double* __restrict__ G, bool active, long long first_k,
                                                     const int (&ix)[kCnt], const int (&iy)[kCnt], const int (&iz)[kCnt], const double (&wx)[3],
                                                     const double (&wy)[3], const double (&wz)[3], double den, unsigned long long& reads) {
    constexpr int kExt = kCnt + 2 * kReach;
    int e[kExt];
#pragma unroll
    for (int j = 0; j < kExt; ++j) e[j] = active ? int(deposit::cell_on_axis(first_k - kReach + j, g.dims[K], g.periodic)) : -1;
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

// ix with the stencil cells dropped whose difference along the axis (first, dim) reads off the grid
template <int kCnt>
__device__ __forceinline__ void drop_unreached(const int (&ix)[kCnt], long long first, int dim, int periodic, int reach, int (&kept)[kCnt]) {
#pragma unroll
    for (int t = 0; t < kCnt; ++t) kept[t] = periodic || (first + t - reach >= 0 && first + t + reach < (long long)dim) ? ix[t] : -1;
}

}  // namespace

template <class F>
__global__ __launch_bounds__(kSampleBlock) void k_sample_stage(const typename Real<F>::V4* __restrict__ pos, const int* __restrict__ count,
                                                               int n_upper, double* __restrict__ xyz) {
    const int i = blockIdx.x * kSampleBlock + threadIdx.x;
    if (i >= live_count(count, n_upper)) return;
    const double4 p = widen(pos[i]);
    xyz[3 * size_t(i)] = p.x;
    xyz[3 * size_t(i) + 1] = p.y;
    xyz[3 * size_t(i) + 2] = p.z;
}

__global__ __launch_bounds__(kSampleBlock) void k_sample_keys(const double* __restrict__ xyz, const int* __restrict__ count, int n,
                                                              deposit::Grid g, uint32_t cells, uint32_t* __restrict__ keys,
                                                              int* __restrict__ rows) {
    const int i = blockIdx.x * kSampleBlock + threadIdx.x;
    if (i >= n) return;
    uint32_t key = cells;
    if (i < (count ? live_count(count, n) : n)) {
        deposit::Stencil st;
        if (deposit::body_stencil(g, xyz[3 * size_t(i)], xyz[3 * size_t(i) + 1], xyz[3 * size_t(i) + 2], 0.0, &st)) key = deposit::home_cell(g, st);
    }
    keys[i] = key;
    rows[i] = i;
}

template <int kReach>
__global__ __launch_bounds__(kSampleBlock) void k_grid_diff(deposit::Grid g, double den, size_t cells, const double* __restrict__ G,
                                                            double* __restrict__ D) {
    const size_t c = size_t(blockIdx.x) * kSampleBlock + threadIdx.x;
    if (c >= cells) return;
    const long long nz = g.dims[2], ny = g.dims[1];
    const long long iz = (long long)c % nz, iy = ((long long)c / nz) % ny, ix = (long long)c / (nz * ny);
    unsigned long long reads = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        double d = 0.0;
        if (k != g.axis && !sample::difference_at(g, G, k, kReach, den, ix, iy, iz, &d, &reads)) d = 0.0;
        D[size_t(k) * cells + c] = d;
    }
}

// rows: the rows in key order [n], or null: lane s takes row s.  G: the grid's fields, or (kModePre) the three difference grids
template <int kMode, int kScheme>
__global__ __launch_bounds__(kSampleBlock) void k_sample(const double* __restrict__ xyz, const int* __restrict__ count, int n, deposit::Grid g,
                                                         int fields, int reach, double den, const double* __restrict__ G,
                                                         const int* __restrict__ rows, double* __restrict__ out, uint8_t* __restrict__ cls_out,
                                                         sample::Words* words) {
    constexpr int kCnt = kScheme + 1;
    const int s = blockIdx.x * kSampleBlock + threadIdx.x;
    const int live = count ? live_count(count, n) : n;
    int row = -1;
    if (s < n) {
        const int r = rows ? rows[s] : s;   // (a permutation of 0 .. n - 1)
        if (r >= 0 && r < live) row = r;
    }
    // (a lane without a row takes the stencil of the grid's corner and drops it: the stencil is then written on every path)
    const double x = row >= 0 ? xyz[3 * size_t(row)] : g.origin[0], y = row >= 0 ? xyz[3 * size_t(row) + 1] : g.origin[1],
                 z = row >= 0 ? xyz[3 * size_t(row) + 2] : g.origin[2];
    deposit::Stencil st;
    const bool taken = deposit::body_stencil(g, x, y, z, 0.0, &st);
    const int cls = row < 0 ? -1 : taken ? sample::point_class(g, st, reach) : int(deposit::kSkipped);
    const bool active = cls == deposit::kInside || cls == deposit::kPartial;
    // the lane's copy of what the terms need, indexed by constants only from here on
    long long f0 = 0, f1 = 0, f2 = 0;
    double wx[3] = {0.0, 0.0, 0.0}, wy[3] = {0.0, 0.0, 0.0}, wz[3] = {0.0, 0.0, 0.0};
    if (active) {
        f0 = st.first[0]; f1 = st.first[1]; f2 = st.first[2];
#pragma unroll
        for (int t = 0; t < 3; ++t) { wx[t] = st.w[0][t]; wy[t] = st.w[1][t]; wz[t] = st.w[2][t]; }
    }
    // the cells an axis has (uniform): kCnt on an axis in use, one on the ignored axis
    const int ca = g.axis == 0 ? 1 : kCnt, cb = g.axis == 1 ? 1 : kCnt, cc = g.axis == 2 ? 1 : kCnt;
    int ix[kCnt], iy[kCnt], iz[kCnt];   // the stencil's indices on the grid, -1: the term is dropped
#pragma unroll
    for (int t = 0; t < kCnt; ++t) {
        ix[t] = active && t < ca ? int(deposit::cell_on_axis(f0 + t, g.dims[0], g.periodic)) : -1;
        iy[t] = active && t < cb ? int(deposit::cell_on_axis(f1 + t, g.dims[1], g.periodic)) : -1;
        iz[t] = active && t < cc ? int(deposit::cell_on_axis(f2 + t, g.dims[2], g.periodic)) : -1;
    }
    unsigned long long reads = 0;
    if constexpr (kMode == kModeValue) {
        const size_t cells = deposit::cells_of(g);
        for (int f = 0; f < fields; ++f) {
            const double sum = weighted_sum<kCnt>(g, G + size_t(f) * cells, ix, iy, iz, wx, wy, wz, reads);
            if (row >= 0) out[size_t(row) * size_t(fields) + f] = sum;
        }
    } else {
        double grad[3] = {0.0, 0.0, 0.0};   // (the component along the ignored axis stays +0.0 and reads nothing)
        if constexpr (kMode == kModePre) {
            const size_t cells = deposit::cells_of(g);
            int kept[kCnt];
            if (g.axis != 0) {
                drop_unreached<kCnt>(ix, f0, g.dims[0], g.periodic, reach, kept);
                grad[0] = weighted_sum<kCnt>(g, G, kept, iy, iz, wx, wy, wz, reads);
            }
            if (g.axis != 1) {
                drop_unreached<kCnt>(iy, f1, g.dims[1], g.periodic, reach, kept);
                grad[1] = weighted_sum<kCnt>(g, G + cells, ix, kept, iz, wx, wy, wz, reads);
            }
            if (g.axis != 2) {
                drop_unreached<kCnt>(iz, f2, g.dims[2], g.periodic, reach, kept);
                grad[2] = weighted_sum<kCnt>(g, G + 2 * cells, ix, iy, kept, wx, wy, wz, reads);
            }
        } else {
            constexpr int kReach = kMode == kModeGrad2 ? 1 : 2;
            if (g.axis != 0) grad[0] = gradient_component<0, kCnt, kReach>(g, G, active, f0, ix, iy, iz, wx, wy, wz, den, reads);
            if (g.axis != 1) grad[1] = gradient_component<1, kCnt, kReach>(g, G, active, f1, ix, iy, iz, wx, wy, wz, den, reads);
            if (g.axis != 2) grad[2] = gradient_component<2, kCnt, kReach>(g, G, active, f2, ix, iy, iz, wx, wy, wz, den, reads);
        }
        if (row >= 0) {
            out[3 * size_t(row)] = grad[0];
            out[3 * size_t(row) + 1] = grad[1];
            out[3 * size_t(row) + 2] = grad[2];
        }
    }
    if (row >= 0) cls_out[row] = uint8_t(cls);
    unsigned long long n_of[4];   // (every lane of the wave is here)
    for (int k = 0; k < 4; ++k) n_of[k] = (unsigned long long)__popcll(__ballot(cls == k));
    if (threadIdx.x % 64 == 0)
        for (int k = 0; k < 4; ++k)
            if (n_of[k]) atomicAdd(&words->counts[k], n_of[k]);
    wave_add(reads, &words->reads);
}

namespace sample {

Plan make_plan(int op, size_t cells) {
    const Tuning& t = nbody::tuning();
    Plan p;
    p.sort = t.sample_sort != 0;
    p.pregrad = t.sample_pregrad != 0 && op != NBODY_SAMPLE_VALUE && 3 * cells <= size_t(NBODY_DEPOSIT_MAX_CELLS);
    return p;
}

namespace {
int key_bits(size_t cells) {   // the bits of the largest key, `cells` itself
    int b = 1;
    while ((size_t(1) << b) <= cells) ++b;
    return b;
}
size_t sort_tmp_bytes(size_t n, size_t cells) {
    size_t b = 0;
    uint32_t* k = nullptr;
    int* v = nullptr;
    (void)rocprim::radix_sort_pairs(nullptr, b, k, k, v, v, n, 0, unsigned(key_bits(cells)), 0);
    return b;
}
Scratch layout(Carver& c, size_t n, size_t cells, int fields, int op, const Plan& p) {
    Scratch w;
    w.words = c.take<Words>(1);
    w.grid = c.take<double>(size_t(fields) * cells);
    if (p.pregrad) w.diff = c.take<double>(3 * cells);
    w.xyz = c.take<double>(3 * n);
    w.out = c.take<double>(size_t(width_of(op, fields)) * n);
    w.cls = c.take<uint8_t>(n);
    if (p.sort) {
        w.keys = c.take<uint32_t>(2 * n);
        w.rows = c.take<int>(2 * n);
        w.sort_bytes = sort_tmp_bytes(n, cells);
        w.sort_tmp = c.take<char>(w.sort_bytes);
    }
    return w;
}
}  // namespace

size_t scratch_bytes(size_t n, size_t cells, int fields, int op, const Plan& p) { Carver c; layout(c, n, cells, fields, op, p); return c.offset(); }
Scratch scratch_layout(void* base, size_t n, size_t cells, int fields, int op, const Plan& p) {
    Carver c(base);
    return layout(c, n, cells, fields, op, p);
}

template <class F>
void launch_stage(hipStream_t s, const ShardT<F>& sh, int n_upper, const Scratch& w) {
    if (n_upper <= 0) return;
    hipLaunchKernelGGL(k_sample_stage<F>, dim3(blocks_for(size_t(n_upper))), dim3(kSampleBlock), 0, s, sh.own_pos(), sh.own_count(), n_upper, w.xyz);
}
template void launch_stage<float>(hipStream_t, const ShardT<float>&, int, const Scratch&);
template void launch_stage<double>(hipStream_t, const ShardT<double>&, int, const Scratch&);

void launch_diff(hipStream_t s, const Grid& g, int op, const Scratch& w) {
    const size_t cells = cells_of(g);
    const double den = denominator_of(op, g.spacing);
    const dim3 grid(blocks_for(cells)), block(kSampleBlock);
    if (op == NBODY_SAMPLE_GRADIENT2) hipLaunchKernelGGL(k_grid_diff<1>, grid, block, 0, s, g, den, cells, w.grid, w.diff);
    else hipLaunchKernelGGL(k_grid_diff<2>, grid, block, 0, s, g, den, cells, w.grid, w.diff);
}

int launch_sample(hipStream_t s, const int* count, int n, const Grid& g, int fields, int op, const Plan& p, const Scratch& w) {
    (void)hipMemsetAsync(w.words, 0, sizeof(Words), s);
    if (n <= 0) return 0;
    const size_t cells = cells_of(g);
    const dim3 grid(blocks_for(size_t(n))), block(kSampleBlock);
    const int* rows = nullptr;
    if (p.sort) {
        hipLaunchKernelGGL(k_sample_keys, grid, block, 0, s, w.xyz, count, n, g, uint32_t(cells), w.keys, w.rows);
        size_t tb = w.sort_bytes;
        if (rocprim::radix_sort_pairs(w.sort_tmp, tb, w.keys, w.keys + n, w.rows, w.rows + n, size_t(n), 0, unsigned(key_bits(cells)), s) != hipSuccess)
            return -1;
        rows = w.rows + n;
    }
    const int mode = op == NBODY_SAMPLE_VALUE ? kModeValue : p.pregrad ? kModePre : op == NBODY_SAMPLE_GRADIENT2 ? kModeGrad2 : kModeGrad4;
    const double* G = mode == kModePre ? w.diff : w.grid;
    const int reach = reach_of(op);
    const double den = denominator_of(op, g.spacing);
#define NBODY_SAMPLE(M, S) \
    hipLaunchKernelGGL((k_sample<M, S>), grid, block, 0, s, w.xyz, count, n, g, fields, reach, den, G, rows, w.out, w.cls, w.words)
#define NBODY_SAMPLE_SCHEMES(M)                                  \
    if (g.scheme == NBODY_DEPOSIT_NGP) NBODY_SAMPLE(M, 0);       \
    else if (g.scheme == NBODY_DEPOSIT_CIC) NBODY_SAMPLE(M, 1);  \
    else NBODY_SAMPLE(M, 2)
    if (mode == kModeValue) { NBODY_SAMPLE_SCHEMES(kModeValue); }
    else if (mode == kModeGrad2) { NBODY_SAMPLE_SCHEMES(kModeGrad2); }
    else if (mode == kModeGrad4) { NBODY_SAMPLE_SCHEMES(kModeGrad4); }
    else { NBODY_SAMPLE_SCHEMES(kModePre); }
#undef NBODY_SAMPLE_SCHEMES
#undef NBODY_SAMPLE
    return 0;
}

}}  // namespace nbody::sample
