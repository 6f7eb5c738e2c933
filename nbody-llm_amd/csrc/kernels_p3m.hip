// kernels_p3m.hip -- the short-range part of nbody_p3m_field and nbody_p3m_field_at on the device (gfx950): a periodic,
// minimum-image pair sum over chain cells (include/nbody_hip.h, "P3M field").  Compiled with -ffp-contract=off; the arithmetic is
// p3m_pairs.h's, and the ORDER of a target's sum is the definition's -- the 27 chain cells dx, dy, dz innermost, ascending row
// within a cell -- whatever the launch shape.  No floating-point atomics.  Every kernel reads the handle's state and writes the
// call's scratch only.
//
//   k_p3m_body_keys<F>  stage[i] = {x, y, z, m} of live row i, widened; key[i] = its chain cell (none, or past the live count:
//                       `cells`, last), row[i] = i
//   k_p3m_point_keys    the same for a batch of caller points, m = 0.0
//   (rocprim::radix_sort_pairs, stable, on (key, row): within a chain cell the rows ascend)
//   k_p3m_gather        sorted[s] = stage[row[s]]: the partner stream of a cell is contiguous
//   k_p3m_starts        start[c] = lower_bound(sorted keys, c) for c = 0 .. cells + 1: the dense cell-start table
//   k_p3m_short<kAtPoints, kLds>  one block per chain cell, which leaves at once when the cell holds no target.  Lanes own the
//                       cell's targets, 128 at a time; for each of the 27 neighbour cells, in the definition's order, the
//                       partners go by 128 at a time -- kLds: staged in LDS as {x, y, z, m} and row, every lane then reads the
//                       same address (a broadcast, no bank conflict); else read from global memory, the cross-check -- and
//                       every lane runs pair_term over them in order.  The split table T stays in global memory: 64 KiB, which
//                       the L2 holds, gathered only by the partners that pass r2 < R2 (at most (4 pi / 3) / 27 = 15.5 % of a uniform stream, when
//                       r_cut = c spacing; the stats' counted / looked is the share of a call).  LDS was not tried for it.  The two pair counts are
//                       per-lane integers, summed across the wave by shuffles and added by one integer atomic per wave.
//   k_p3m_add           acc = acc_mesh + acc_short, phi = phi_mesh + phi_short (SHORT_ONLY: the short part alone)
#include "kernels_p3m.h"
#include "device_util.h"
#include "kernels.h"   // tuning()
#include "real.h"      // widen
#include "scratch_carve.h"

#include <rocprim/device/device_radix_sort.hpp>

namespace nbody {

using p3m::kP3mBlock;

namespace {
constexpr int kRowBlock = 256;
inline int row_blocks(size_t n) { return int((n + kRowBlock - 1) / kRowBlock); }
}  // namespace

template <class F>
__global__ __launch_bounds__(kRowBlock) void k_p3m_body_keys(const typename Real<F>::V4* __restrict__ pos, const int* __restrict__ count, int n_upper,
                                                             deposit::Grid g, p3m::Chain ch, uint32_t cells, double4* __restrict__ stage,
                                                             uint32_t* __restrict__ keys, int* __restrict__ rows) {
    const int i = blockIdx.x * kRowBlock + threadIdx.x;
    if (i >= n_upper) return;
    uint32_t key = cells;
    if (i < live_count(count, n_upper)) {
        const double4 p = widen(pos[i]);
        stage[i] = p;
        uint32_t c;
        if (p3m::chain_cell(g, ch, p.x, p.y, p.z, p.w, &c)) key = c;
    }
    keys[i] = key;
    rows[i] = i;
}

__global__ __launch_bounds__(kRowBlock) void k_p3m_point_keys(const double* __restrict__ xyz, int n, deposit::Grid g, p3m::Chain ch, uint32_t cells,
                                                              double4* __restrict__ stage, uint32_t* __restrict__ keys, int* __restrict__ rows) {
    const int i = blockIdx.x * kRowBlock + threadIdx.x;
    if (i >= n) return;
    const double4 p = make_double4(xyz[3 * size_t(i)], xyz[3 * size_t(i) + 1], xyz[3 * size_t(i) + 2], 0.0);
    stage[i] = p;
    uint32_t c, key = cells;
    if (p3m::chain_cell(g, ch, p.x, p.y, p.z, 0.0, &c)) key = c;
    keys[i] = key;
    rows[i] = i;
}

// (a row past the live count was never staged: its key is `cells`, no start below cells + 1 reaches it and nobody reads its copy)
__global__ __launch_bounds__(kRowBlock) void k_p3m_gather(const double4* __restrict__ stage, const int* __restrict__ rows, int n,
                                                          double4* __restrict__ sorted) {
    const int s = blockIdx.x * kRowBlock + threadIdx.x;
    if (s < n) sorted[s] = stage[rows[s]];
}

__global__ __launch_bounds__(kRowBlock) void k_p3m_starts(const uint32_t* __restrict__ keys, int n, uint32_t cells, int* __restrict__ start) {
    const uint32_t c = blockIdx.x * kRowBlock + threadIdx.x;
    if (c > cells + 1) return;
    int lo = 0, hi = n;   // the first place whose key is >= c
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (keys[mid] < c) lo = mid + 1;
        else hi = mid;
    }
    start[c] = lo;
}

template <bool kAtPoints, bool kLds>
__global__ __launch_bounds__(kP3mBlock) void k_p3m_short(const double4* __restrict__ partners, const int* __restrict__ partner_rows,
                                                         const int* __restrict__ partner_start, const double4* __restrict__ targets,
                                                         const int* __restrict__ target_rows, const int* __restrict__ target_start, p3m::Chain ch,
                                                         p3m::Params p, double g, const p3m::Entry* __restrict__ T, double4* __restrict__ out,
                                                         p3m::Words* words) {
    const uint32_t cell = blockIdx.x;
    const int t0 = target_start[cell], t1 = target_start[cell + 1];
    if (t0 == t1) return;   // (the whole block)
    __shared__ double4 sp[kLds ? kP3mBlock : 1];
    __shared__ int sr[kLds ? kP3mBlock : 1];
    const int tid = threadIdx.x;
    unsigned long long looked = 0, counted = 0;
    for (int tile = t0; tile < t1; tile += kP3mBlock) {
        const bool live = tile + tid < t1;
        const double4 me = live ? targets[tile + tid] : make_double4(0.0, 0.0, 0.0, 0.0);
        const int my_row = live ? target_rows[tile + tid] : -1;
        p3m::Sums s;
        for (int q = 0; q < 27; ++q) {
            const uint32_t c = p3m::chain_neighbour(ch, cell, q);
            const int j0 = partner_start[c], j1 = partner_start[c + 1];   // (the same for every lane of the block)
            for (int base = j0; base < j1; base += kP3mBlock) {
                const int cnt = min(kP3mBlock, j1 - base);
                if constexpr (kLds) {
                    __syncthreads();   // the lanes have done with the partners staged before
                    if (tid < cnt) {
                        sp[tid] = partners[base + tid];
                        sr[tid] = partner_rows[base + tid];
                    }
                    __syncthreads();
                }
                if (!live) continue;
                for (int k = 0; k < cnt; ++k) {
                    const double4 pj = kLds ? sp[k] : partners[base + k];
                    if constexpr (!kAtPoints) {
                        if ((kLds ? sr[k] : partner_rows[base + k]) == my_row) continue;
                    }
                    p3m::pair_term(p, T, me.x, me.y, me.z, pj.x, pj.y, pj.z, pj.w, s);
                }
            }
        }
        if (live) {
            double row[4];
            p3m::short_row(g, s, row);
            out[my_row] = make_double4(row[0], row[1], row[2], row[3]);
        }
        looked += s.looked;
        counted += s.counted;
    }
    for (int off = 32; off > 0; off >>= 1) {
        looked += __shfl_down(looked, off, 64);
        counted += __shfl_down(counted, off, 64);
    }
    if ((tid & 63) == 0) {
        if (looked) atomicAdd(&words->looked, looked);
        if (counted) atomicAdd(&words->counted, counted);
    }
}

__global__ __launch_bounds__(kRowBlock) void k_p3m_add(const int* __restrict__ count, int n, int short_only, const double4* __restrict__ part,
                                                       double* __restrict__ acc, double* __restrict__ phi) {
    const int i = blockIdx.x * kRowBlock + threadIdx.x;
    if (i >= (count ? live_count(count, n) : n)) return;
    const double4 s = part[i];
    double* a = acc + 3 * size_t(i);
    a[0] = short_only ? s.x : a[0] + s.x;
    a[1] = short_only ? s.y : a[1] + s.y;
    a[2] = short_only ? s.z : a[2] + s.z;
    if (phi) phi[i] = short_only ? s.w : phi[i] + s.w;
}

namespace p3m {

Plan make_plan() {
    Plan p;
    p.lds = nbody::tuning().p3m_lds != 0;
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
Order order_layout(Carver& c, size_t n, size_t cells) {
    Order o;
    o.stage = c.take<double4>(n);
    o.sorted = c.take<double4>(n);
    o.keys = c.take<uint32_t>(2 * n);
    o.rows = c.take<int>(2 * n);
    o.start = c.take<int>(cells + 2);
    return o;
}
Scratch layout(Carver& c, size_t n_bodies, size_t n_rows, size_t cells, bool at_points) {
    Scratch w;
    w.table = c.take<Entry>(size_t(kIntervals) + 1);
    w.words = c.take<Words>(1);
    w.bodies = order_layout(c, n_bodies, cells);
    if (at_points) w.pts = order_layout(c, n_rows, cells);
    w.out = c.take<double4>(n_rows);
    w.sort_bytes = sort_tmp_bytes(std::max(n_bodies, at_points ? n_rows : size_t(0)), cells);
    w.sort_tmp = c.take<char>(w.sort_bytes);
    return w;
}

// the sort, the gather and the starts of an order whose keys and rows are made
int finish_order(hipStream_t s, int n, const Chain& ch, const Order& o, const Scratch& w) {
    const uint32_t cells = uint32_t(ch.cells());
    size_t tb = w.sort_bytes;   // (sized for the larger of the two orders: rocPRIM's temporary size does not fall as n grows, as the other grid calls assume)
    if (rocprim::radix_sort_pairs(w.sort_tmp, tb, o.keys, o.keys + n, o.rows, o.rows + n, size_t(n), 0, unsigned(key_bits(cells)), s) != hipSuccess)
        return -1;
    hipLaunchKernelGGL(k_p3m_gather, dim3(row_blocks(size_t(n))), dim3(kRowBlock), 0, s, o.stage, o.rows + n, n, o.sorted);
    hipLaunchKernelGGL(k_p3m_starts, dim3(row_blocks(size_t(cells) + 2)), dim3(kRowBlock), 0, s, o.keys + n, n, cells, o.start);
    return 0;
}
}  // namespace

size_t scratch_bytes(size_t n_bodies, size_t n_rows, size_t chain_cells, bool at_points) {
    Carver c;
    layout(c, n_bodies, n_rows, chain_cells, at_points);
    return c.offset();
}
Scratch scratch_layout(void* base, size_t n_bodies, size_t n_rows, size_t chain_cells, bool at_points) {
    Carver c(base);
    return layout(c, n_bodies, n_rows, chain_cells, at_points);
}

template <class F>
int launch_body_order(hipStream_t s, const ShardT<F>& sh, int n_upper, const deposit::Grid& g, const Chain& ch, const Scratch& w) {
    const uint32_t cells = uint32_t(ch.cells());
    if (n_upper <= 0) {   // no body: every cell starts and ends at 0
        (void)hipMemsetAsync(w.bodies.start, 0, (size_t(cells) + 2) * sizeof(int), s);
        return 0;
    }
    hipLaunchKernelGGL(k_p3m_body_keys<F>, dim3(row_blocks(size_t(n_upper))), dim3(kRowBlock), 0, s, sh.own_pos(), sh.own_count(), n_upper, g, ch, cells,
                       w.bodies.stage, w.bodies.keys, w.bodies.rows);
    return finish_order(s, n_upper, ch, w.bodies, w);
}
template int launch_body_order<float>(hipStream_t, const ShardT<float>&, int, const deposit::Grid&, const Chain&, const Scratch&);
template int launch_body_order<double>(hipStream_t, const ShardT<double>&, int, const deposit::Grid&, const Chain&, const Scratch&);

int launch_point_order(hipStream_t s, const double* xyz, int n, const deposit::Grid& g, const Chain& ch, const Scratch& w) {
    const uint32_t cells = uint32_t(ch.cells());
    if (n <= 0) {
        (void)hipMemsetAsync(w.pts.start, 0, (size_t(cells) + 2) * sizeof(int), s);
        return 0;
    }
    hipLaunchKernelGGL(k_p3m_point_keys, dim3(row_blocks(size_t(n))), dim3(kRowBlock), 0, s, xyz, n, g, ch, cells, w.pts.stage, w.pts.keys, w.pts.rows);
    return finish_order(s, n, ch, w.pts, w);
}

void launch_short(hipStream_t s, int n_bodies, int n_rows, bool at_points, const Plan& plan, const Chain& ch, const Params& p, double g,
                  const Scratch& w) {
    if (n_rows <= 0) return;
    (void)hipMemsetAsync(w.out, 0, size_t(n_rows) * sizeof(double4), s);   // (+0.0 four times: a target without a chain cell)
    const dim3 grid(unsigned(ch.cells())), block(kP3mBlock);
    const Order& t = at_points ? w.pts : w.bodies;
    const int* partner_rows = w.bodies.rows + n_bodies;   // (the sorted halves)
    const int* target_rows = at_points ? w.pts.rows + n_rows : partner_rows;
    const auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, block, 0, s, w.bodies.sorted, partner_rows, w.bodies.start, t.sorted, target_rows, t.start, ch, p, g, w.table,
                           w.out, w.words);
    };
    if (at_points) {
        if (plan.lds) launch(k_p3m_short<true, true>);
        else launch(k_p3m_short<true, false>);
    } else {
        if (plan.lds) launch(k_p3m_short<false, true>);
        else launch(k_p3m_short<false, false>);
    }
}

void launch_add(hipStream_t s, const int* count, int n, int terms, const Scratch& w, double* acc, double* phi) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_p3m_add, dim3(row_blocks(size_t(n))), dim3(kRowBlock), 0, s, count, n, terms == NBODY_P3M_SHORT_ONLY ? 1 : 0, w.out, acc, phi);
}

}}  // namespace nbody::p3m
