// kernels_pm.hip -- nbody_pm_field and nbody_pm_field_at on the device (gfx950): the scratch that the deposit, the Poisson solve
// and the gather share, and the gather itself (include/nbody_hip.h, "particle-mesh field").  Compiled with -ffp-contract=off.
// The deposit and the solve are kernels_deposit.hip's and kernels_poisson.hip's launches as they stand; what is new is
//
//   k_pm_gather<kReach, kScheme>  one lane per place of the home-cell order (or per row, unsorted).  ONE stencil set-up
//                   (sample_device.h LaneStencil) gives the three components of acc and phi together.  Every output is the
//                   expression tree of the matching k_sample instance, because it calls the same functions of sample_device.h:
//                   gradient_component<K> for the components, and for phi weighted_sum's terms in weighted_sum's order -- summed,
//                   for CIC and TSC, over the middle kCnt planes that gradient_component<0> has loaded anyway (kWithValue), so
//                   phi costs no further grid read; NGP reads its own cell once more (no difference reads it), and a grid whose
//                   ignored axis is x has no x component to borrow from and calls weighted_sum.  acc = 0.0 - grad, so that a zero
//                   is +0.0.  with_phi == 0: no value sum, no phi store.  The counts come from ballots and one integer atomic
//                   per wave and class.  No floating-point atomics, no LDS, no lane ever waits for another.
//   k_pm_negate     pm_gather = 0: the gradient rows of k_sample become acc in place
#include "kernels_pm.h"
#include "sample_device.h"
#include "kernels.h"   // tuning()
#include "scratch_carve.h"

namespace nbody {

using sample::kSampleBlock;

template <int kReach, int kScheme>
__global__ __launch_bounds__(kSampleBlock) void k_pm_gather(const double* __restrict__ xyz, const int* __restrict__ count, int n, deposit::Grid g,
                                                            double den, const double* __restrict__ G, const int* __restrict__ rows, int with_phi,
                                                            double* __restrict__ acc, double* __restrict__ phi, uint8_t* __restrict__ cls_out,
                                                            sample::Words* words) {
    constexpr int kCnt = kScheme + 1;
    sample::LaneStencil<kCnt> lane;
    lane.set_up(xyz, count, n, g, kReach, rows, blockIdx.x * kSampleBlock + threadIdx.x);
    unsigned long long reads = 0;
    double grad[3] = {0.0, 0.0, 0.0}, value = 0.0;   // (the component along the ignored axis stays +0.0 and reads nothing)
    if (g.axis != 0) {
        if constexpr (kCnt > 1) {
            if (with_phi) grad[0] = sample::gradient_component<0, kCnt, kReach, true>(g, G, lane, den, reads, &value);
            else grad[0] = sample::gradient_component<0, kCnt, kReach>(g, G, lane, den, reads);
        } else {
            grad[0] = sample::gradient_component<0, kCnt, kReach>(g, G, lane, den, reads);
        }
    }
    if (with_phi && (kCnt == 1 || g.axis == 0)) value = sample::weighted_sum<kCnt>(g, G, lane.ix, lane.iy, lane.iz, lane.wx, lane.wy, lane.wz, reads);
    if (g.axis != 1) grad[1] = sample::gradient_component<1, kCnt, kReach>(g, G, lane, den, reads);
    if (g.axis != 2) grad[2] = sample::gradient_component<2, kCnt, kReach>(g, G, lane, den, reads);
    const int row = lane.row;
    if (row >= 0) {
        acc[3 * size_t(row)] = 0.0 - grad[0];
        acc[3 * size_t(row) + 1] = 0.0 - grad[1];
        acc[3 * size_t(row) + 2] = 0.0 - grad[2];
        if (with_phi) phi[row] = value;
        cls_out[row] = uint8_t(lane.cls);
    }
    sample::count_classes(lane.cls, reads, words);
}

__global__ __launch_bounds__(kSampleBlock) void k_pm_negate(const int* __restrict__ count, int n, double* __restrict__ rows) {
    const size_t i = size_t(blockIdx.x) * kSampleBlock + threadIdx.x;
    const int live = count ? live_count(count, n) : n;
    if (i < 3 * size_t(live)) rows[i] = 0.0 - rows[i];
}

namespace pm {

Plan make_plan() {
    const Tuning& t = nbody::tuning();
    Plan p;
    p.gather = t.pm_gather != 0;
    p.share_sort = t.pm_share_sort != 0;
    return p;
}

Plans make_plans(int gradient_op, size_t cells, bool at_bodies) {
    Plans p;
    p.pm = make_plan();
    p.dep = deposit::make_plan();
    p.poi = poisson::make_plan();
    p.grad = sample::make_plan(gradient_op, cells);
    if (p.pm.gather) p.grad.pregrad = 0;   // (k_pm_gather forms the differences on the fly)
    p.value = sample::make_plan(NBODY_SAMPLE_VALUE, cells);
    p.shared = at_bodies && p.pm.share_sort && p.dep.sort && p.grad.sort;
    return p;
}

namespace {
Scratch layout(Carver& c, void* base, size_t n_bodies, size_t n_rows, const deposit::Grid& g, const poisson::Shape& sh, bool deconvolve,
               int gradient_op, const Plans& p) {
    const size_t cells = deposit::cells_of(g);
    const bool dep_sorts = p.dep.sort && !p.shared;
    Scratch w;
    // the three stages' own descriptions, one after the other (each a multiple of 256 bytes); the Poisson stage and the sampler
    // take no grid of their own
    const size_t b_dep = deposit::scratch_bytes(n_bodies, cells, true, dep_sorts), b_poi = poisson::scratch_bytes(sh, deconvolve, false),
                 b_smp = sample::scratch_bytes(n_rows, cells, 1, gradient_op, p.grad, false);
    char* dep = c.take<char>(b_dep);
    char* poi = c.take<char>(b_poi);
    char* smp = c.take<char>(b_smp);
    w.phi = c.take<double>(n_rows);
    if (!p.pm.gather) {
        w.value_words = c.take<sample::Words>(1);
        w.value_cls = c.take<uint8_t>(n_rows);
    }
    if (!base) return w;   // (measuring)
    w.dep = deposit::scratch_layout(dep, n_bodies, cells, true, dep_sorts);
    w.poi = poisson::scratch_layout(poi, sh, deconvolve, false);
    w.smp = sample::scratch_layout(smp, n_rows, cells, 1, gradient_op, p.grad, false);
    w.poi.real = reinterpret_cast<double*>(w.dep.acc);   // the same eight bytes a cell: sums, then mass, then phi
    w.smp.grid = w.poi.real;
    return w;
}
}  // namespace

size_t scratch_bytes(size_t n_bodies, size_t n_rows, const deposit::Grid& g, const poisson::Shape& sh, bool deconvolve, int gradient_op,
                     const Plans& p) {
    Carver c;
    layout(c, nullptr, n_bodies, n_rows, g, sh, deconvolve, gradient_op, p);
    return c.offset();
}
Scratch scratch_layout(void* base, size_t n_bodies, size_t n_rows, const deposit::Grid& g, const poisson::Shape& sh, bool deconvolve,
                       int gradient_op, const Plans& p) {
    Carver c(base);
    return layout(c, base, n_bodies, n_rows, g, sh, deconvolve, gradient_op, p);
}

void launch_gather(hipStream_t s, const int* count, int n, const deposit::Grid& g, int gradient_op, bool with_phi, const int* rows, const Scratch& w) {
    (void)hipMemsetAsync(w.smp.words, 0, sizeof(sample::Words), s);
    if (n <= 0) return;
    const dim3 grid(sample::blocks_for(size_t(n))), block(kSampleBlock);
    const double den = sample::denominator_of(gradient_op, g.spacing);
    sample::for_reach_and_scheme(gradient_op, g.scheme, [&](auto reach, auto scheme) {
        hipLaunchKernelGGL((k_pm_gather<decltype(reach)::value, decltype(scheme)::value>), grid, block, 0, s, w.smp.xyz, count, n, g, den, w.smp.grid,
                           rows, with_phi ? 1 : 0, w.smp.out, w.phi, w.smp.cls, w.smp.words);
    });
}

void launch_negate(hipStream_t s, const int* count, int n, double* rows) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_pm_negate, dim3(sample::blocks_for(3 * size_t(n))), dim3(kSampleBlock), 0, s, count, n, rows);
}

}}  // namespace nbody::pm
