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
//                   2 reach cnt.  The counts come from ballots and one integer atomic per wave and class.  The stencil set-up,
//                   the sums, the gradient and the counts are sample_device.h's, which says who else calls them.
#include "kernels_sample.h"
#include "sample_device.h"
#include "kernels.h"   // tuning()
#include "real.h"      // widen
#include "scratch_carve.h"

#include <rocprim/device/device_radix_sort.hpp>

namespace nbody {

using sample::kSampleBlock;
using sample::count_classes;
using sample::drop_unreached;
using sample::weighted_sum;

namespace {

enum { kModeValue = 0, kModeGrad2 = 1, kModeGrad4 = 2, kModePre = 3 };

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
    sample::LaneStencil<kCnt> lane;   // (sample_device.h: the row, the class and the stencil, indexed by constants only)
    lane.set_up(xyz, count, n, g, reach, rows, blockIdx.x * kSampleBlock + threadIdx.x);
    const int row = lane.row, cls = lane.cls;
    unsigned long long reads = 0;
    if constexpr (kMode == kModeValue) {
        const size_t cells = deposit::cells_of(g);
        for (int f = 0; f < fields; ++f) {
            const double sum = weighted_sum<kCnt>(g, G + size_t(f) * cells, lane.ix, lane.iy, lane.iz, lane.wx, lane.wy, lane.wz, reads);
            if (row >= 0) out[size_t(row) * size_t(fields) + f] = sum;
        }
    } else {
        double grad[3] = {0.0, 0.0, 0.0};   // (the component along the ignored axis stays +0.0 and reads nothing)
        if constexpr (kMode == kModePre) {
            const size_t cells = deposit::cells_of(g);
            int kept[kCnt];
            if (g.axis != 0) {
                drop_unreached<kCnt>(lane.ix, lane.f0, g.dims[0], g.periodic, reach, kept);
                grad[0] = weighted_sum<kCnt>(g, G, kept, lane.iy, lane.iz, lane.wx, lane.wy, lane.wz, reads);
            }
            if (g.axis != 1) {
                drop_unreached<kCnt>(lane.iy, lane.f1, g.dims[1], g.periodic, reach, kept);
                grad[1] = weighted_sum<kCnt>(g, G + cells, lane.ix, kept, lane.iz, lane.wx, lane.wy, lane.wz, reads);
            }
            if (g.axis != 2) {
                drop_unreached<kCnt>(lane.iz, lane.f2, g.dims[2], g.periodic, reach, kept);
                grad[2] = weighted_sum<kCnt>(g, G + 2 * cells, lane.ix, lane.iy, kept, lane.wx, lane.wy, lane.wz, reads);
            }
        } else {
            sample::lane_gradient<kCnt, kMode == kModeGrad2 ? 1 : 2>(g, G, lane, den, reads, grad);
        }
        if (row >= 0) {
            out[3 * size_t(row)] = grad[0];
            out[3 * size_t(row) + 1] = grad[1];
            out[3 * size_t(row) + 2] = grad[2];
        }
    }
    if (row >= 0) cls_out[row] = uint8_t(cls);
    count_classes(cls, reads, words);
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
Scratch layout(Carver& c, size_t n, size_t cells, int fields, int op, const Plan& p, bool own_grid) {
    Scratch w;
    w.words = c.take<Words>(1);
    if (own_grid) w.grid = c.take<double>(size_t(fields) * cells);
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

size_t scratch_bytes(size_t n, size_t cells, int fields, int op, const Plan& p, bool own_grid) {
    Carver c;
    layout(c, n, cells, fields, op, p, own_grid);
    return c.offset();
}
Scratch scratch_layout(void* base, size_t n, size_t cells, int fields, int op, const Plan& p, bool own_grid) {
    Carver c(base);
    return layout(c, n, cells, fields, op, p, own_grid);
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

int launch_order(hipStream_t s, const int* count, int n, const Grid& g, const Scratch& w) {
    if (n <= 0) return 0;
    const size_t cells = cells_of(g);
    hipLaunchKernelGGL(k_sample_keys, dim3(blocks_for(size_t(n))), dim3(kSampleBlock), 0, s, w.xyz, count, n, g, uint32_t(cells), w.keys, w.rows);
    size_t tb = w.sort_bytes;
    return rocprim::radix_sort_pairs(w.sort_tmp, tb, w.keys, w.keys + n, w.rows, w.rows + n, size_t(n), 0, unsigned(key_bits(cells)), s) == hipSuccess ? 0 : -1;
}

const int* ordered_rows(hipStream_t s, const int* count, int n, const Grid& g, const Scratch& w, bool sort, bool ordered, int* rc, uint64_t* sorts) {
    *rc = sort && !ordered ? launch_order(s, count, n, g, w) : 0;
    if (sort && !ordered && *rc == 0 && sorts) ++*sorts;
    return sort ? w.rows + n : nullptr;
}

int launch_sample(hipStream_t s, const int* count, int n, const Grid& g, int fields, int op, const Plan& p, const Scratch& w, bool ordered) {
    (void)hipMemsetAsync(w.words, 0, sizeof(Words), s);
    if (n <= 0) return 0;
    const dim3 grid(blocks_for(size_t(n))), block(kSampleBlock);
    int rc = 0;
    const int* rows = ordered_rows(s, count, n, g, w, p.sort != 0, ordered, &rc);
    if (rc) return -1;
    const int mode = op == NBODY_SAMPLE_VALUE ? kModeValue : p.pregrad ? kModePre : op == NBODY_SAMPLE_GRADIENT2 ? kModeGrad2 : kModeGrad4;
    const double* G = mode == kModePre ? w.diff : w.grid;
    const int reach = reach_of(op);
    const double den = denominator_of(op, g.spacing);
    const auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, block, 0, s, w.xyz, count, n, g, fields, reach, den, G, rows, w.out, w.cls, w.words);
    };
    switch (mode) {
    case kModeValue: for_scheme(g.scheme, [&](auto sc) { launch(k_sample<kModeValue, decltype(sc)::value>); }); break;
    case kModePre: for_scheme(g.scheme, [&](auto sc) { launch(k_sample<kModePre, decltype(sc)::value>); }); break;
    default:   // kModeGrad2 | kModeGrad4: the op is a gradient operator
        for_reach_and_scheme(op, g.scheme, [&](auto r, auto sc) {
            launch(k_sample<decltype(r)::value == 1 ? kModeGrad2 : kModeGrad4, decltype(sc)::value>);
        });
    }
    return 0;
}

}}  // namespace nbody::sample
