// kernels_deposit.hip -- nbody_deposit on the device (gfx950): the bodies of a handle assigned to a regular grid, NGP / CIC /
// TSC, in 64-bit fixed point (include/nbody_hip.h, "grid deposit").  Compiled with -ffp-contract=off; the arithmetic is
// deposit_grid.h's.  No floating-point atomics: every sum is an integer sum, so neither the order of the bodies nor the way
// the additions are grouped can show.  No lane ever waits for another wave or workgroup.  Every kernel reads the handle's
// state and writes the call's scratch only.
//
//   k_deposit_q        q of every live row; the largest |q| among the bodies that are not skipped (non-negative doubles order
//                      as their bits: shuffles, then one integer atomicMax per wave); the four counts (ballots, then one
//                      atomicAdd per wave and class)
//   k_deposit_keys     key[i] = the home cell of row i (rows past the live count and skipped bodies: `cells`, last), row[i] = i
//   (rocprim::radix_sort_pairs, stable, on (key, row): the bodies cell after cell)
//   k_deposit          one lane per place of that order (or per row, unsorted).  The stencil offsets are walked in one order by
//                      every lane, so at one offset the lanes of a wave that share a home cell hit the same cell and stand in a
//                      run.  kCombine: a segmented inclusive scan over the runs by shuffles (the run's first lane from a
//                      ballot of the heads) leaves each run's sum in its last lane, which alone adds it.  kLds: the addition
//                      goes to the block's table of kTileSlots tagged int64 slots in LDS -- slot = cell mod kTileSlots, claimed
//                      with an LDS compare-and-swap on the tag; a slot that another cell holds sends the addition to global
//                      memory -- and the table is added to the cells at the block's end.  Otherwise one 64-bit vector atomic,
//                      relaxed, agent scope, to the cell.  Sums that are zero are not sent.
//   k_deposit_convert  grid[c] = ldexp((double) acc[c], -S), in place
// S is formed on the device from the live count and the largest |q| (deposit_grid.h scale_of): no host round trip in between.
#include "kernels_deposit.h"
#include "device_util.h"   // live_count, wave_add
#include "kernels.h"   // tuning()
#include "real.h"      // widen
#include "scratch_carve.h"

#include <rocprim/device/device_radix_sort.hpp>

namespace nbody {

using deposit::kDepositBlock;
using deposit::kTileSlots;

namespace {

__device__ __forceinline__ double quantity_of(int quantity, const double4 p, const double4 v) {
    switch (quantity) {
    case NBODY_DEPOSIT_MASS: return p.w;
    case NBODY_DEPOSIT_MOMENTUM_X: return p.w * v.x;
    case NBODY_DEPOSIT_MOMENTUM_Y: return p.w * v.y;
    case NBODY_DEPOSIT_MOMENTUM_Z: return p.w * v.z;
    case NBODY_DEPOSIT_MV2: return p.w * ((v.x * v.x + v.y * v.y) + v.z * v.z);
    default: return 1.0;
    }
}

__device__ __forceinline__ void global_add(long long* acc, long long cell, unsigned long long v, unsigned long long& issued) {
    (void)__hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(acc) + cell, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    ++issued;
}

// v into cell (cell < 0: this lane adds nothing).  Every lane of the wave calls it together.
template <bool kCombine, bool kLds>
__device__ __forceinline__ void add_term(long long cell, unsigned long long v, int* tags, unsigned long long* sums, long long* acc,
                                         unsigned long long& issued) {
    bool emit = cell >= 0;
    if constexpr (kCombine) {
        const int lane = int(threadIdx.x) % 64;
        const long long before = __shfl_up(cell, 1, 64), after = __shfl_down(cell, 1, 64);
        const unsigned long long heads = __ballot(lane == 0 || before != cell);
        const int start = 63 - __builtin_clzll(heads & (~0ull >> (63 - lane)));   // the run's first lane (bit 0 is always set)
        for (int off = 1; off < 64; off <<= 1) {   // segmented inclusive scan: lanes of one run only
            const unsigned long long u = __shfl_up(v, off, 64);
            if (lane - off >= start) v += u;
        }
        emit = emit && (lane == 63 || after != cell);   // the run's last lane holds its sum
    }
    if (!emit || !v) return;
    if constexpr (kLds) {
        const int slot = int(cell & (kTileSlots - 1));
        const int held = atomicCAS(tags + slot, -1, int(cell));
        if (held == -1 || held == int(cell)) {
            atomicAdd(sums + slot, v);   // (an LDS integer atomic)
            return;
        }
    }
    global_add(acc, cell, v, issued);
}

}  // namespace

template <class F>
__global__ __launch_bounds__(kDepositBlock) void k_deposit_q(const typename Real<F>::V4* __restrict__ pos,
                                                             const typename Real<F>::V4* __restrict__ vel, const int* __restrict__ count,
                                                             int n_upper, deposit::Grid g, int quantity, double* __restrict__ q,
                                                             deposit::Words* words) {
    const int i = blockIdx.x * kDepositBlock + threadIdx.x;
    int cls = -1;
    unsigned long long bits = 0;
    if (i < live_count(count, n_upper)) {
        const double4 p = widen(pos[i]);
        const double qv = quantity_of(quantity, p, widen(vel[i]));
        q[i] = qv;
        deposit::Stencil st;
        if (deposit::body_stencil(g, p.x, p.y, p.z, qv, &st)) {
            cls = deposit::body_class(st);
            bits = (unsigned long long)__double_as_longlong(fabs(qv));
        } else {
            cls = deposit::kSkipped;
        }
    }
    for (int off = 32; off >= 1; off >>= 1) {   // (every lane of the wave is here)
        const unsigned long long o = __shfl_xor(bits, off, 64);
        bits = o > bits ? o : bits;
    }
    unsigned long long n_of[4];
    for (int k = 0; k < 4; ++k) n_of[k] = (unsigned long long)__popcll(__ballot(cls == k));
    if (threadIdx.x % 64 == 0) {
        if (bits) atomicMax(&words->qmax_bits, bits);
        for (int k = 0; k < 4; ++k)
            if (n_of[k]) atomicAdd(&words->counts[k], n_of[k]);
    }
}

template <class F>
__global__ __launch_bounds__(kDepositBlock) void k_deposit_keys(const typename Real<F>::V4* __restrict__ pos, const int* __restrict__ count,
                                                                int n_upper, deposit::Grid g, uint32_t cells, const double* __restrict__ q,
                                                                uint32_t* __restrict__ keys, int* __restrict__ rows) {
    const int i = blockIdx.x * kDepositBlock + threadIdx.x;
    if (i >= n_upper) return;
    uint32_t key = cells;
    if (i < live_count(count, n_upper)) {
        const double4 p = widen(pos[i]);
        deposit::Stencil st;
        if (deposit::body_stencil(g, p.x, p.y, p.z, q[i], &st)) key = deposit::home_cell(g, st);
    }
    keys[i] = key;
    rows[i] = i;
}

// rows: the rows in key order [n_upper], or null: lane s takes row s
template <class F, bool kCombine, bool kLds>
__global__ __launch_bounds__(kDepositBlock) void k_deposit(const typename Real<F>::V4* __restrict__ pos, const int* __restrict__ count,
                                                           int n_upper, deposit::Grid g, const double* __restrict__ q,
                                                           const int* __restrict__ rows, deposit::Words* words, long long* acc) {
    __shared__ unsigned long long sums[kLds ? kTileSlots : 1];
    __shared__ int tags[kLds ? kTileSlots : 1];
    if constexpr (kLds) {
        for (int k = threadIdx.x; k < kTileSlots; k += kDepositBlock) { sums[k] = 0ull; tags[k] = -1; }
        __syncthreads();
    }
    const int s = blockIdx.x * kDepositBlock + threadIdx.x;
    const int live = live_count(count, n_upper);
    const int S = deposit::scale_of((unsigned long long)live, __longlong_as_double((long long)words->qmax_bits));
    deposit::Stencil st = {};
    bool active = false;
    double qv = 0.0;
    if (s < n_upper) {
        const int row = rows ? rows[s] : s;   // (a permutation of 0 .. n_upper - 1)
        if (row < live) {
            const double4 p = widen(pos[row]);
            qv = q[row];
            active = deposit::body_stencil(g, p.x, p.y, p.z, qv, &st);
        }
    }
    // the lane's copy of what the terms need, indexed by constants only from here on
    const long long f0 = st.first[0], f1 = st.first[1], f2 = st.first[2];
    const double wx[3] = {st.w[0][0], st.w[0][1], st.w[0][2]}, wy[3] = {st.w[1][0], st.w[1][1], st.w[1][2]},
                 wz[3] = {st.w[2][0], st.w[2][1], st.w[2][2]};
    // the offsets every lane walks (uniform): scheme + 1 cells on an axis in use, one on the ignored axis
    const int per_axis = g.scheme + 1;
    const int ca = g.axis == 0 ? 1 : per_axis, cb = g.axis == 1 ? 1 : per_axis, cc = g.axis == 2 ? 1 : per_axis;
    unsigned long long issued = 0, terms = 0;
    // the 27 offsets written out: every index into the stencil is a constant, so it stays in registers
#define NBODY_DEPOSIT_TERM(A, B, C)                                                                                                  \
    if (A < ca && B < cb && C < cc) { /* (uniform: every lane of the block walks the same offsets) */                                 \
        long long cell = -1;                                                                                                         \
        unsigned long long k = 0;                                                                                                    \
        if (active) {                                                                                                                \
            const long long ix = deposit::cell_on_axis(f0 + A, g.dims[0], g.periodic),                                      \
                            iy = deposit::cell_on_axis(f1 + B, g.dims[1], g.periodic),                                      \
                            iz = deposit::cell_on_axis(f2 + C, g.dims[2], g.periodic);                                      \
            if (ix >= 0 && iy >= 0 && iz >= 0) {                                                                                     \
                const double t = qv * ((wx[A] * wy[B]) * wz[C]);                                                                      \
                k = (unsigned long long)deposit::fixed_of(t, S);                                                                     \
                cell = (ix * (long long)g.dims[1] + iy) * (long long)g.dims[2] + iz; /* (< dims' product <= 2^27) */                  \
                ++terms;                                                                                                             \
            }                                                                                                                        \
        }                                                                                                                            \
        add_term<kCombine, kLds>(cell, k, tags, sums, acc, issued);                                                                  \
    }
#define NBODY_DEPOSIT_ROW(A, B) NBODY_DEPOSIT_TERM(A, B, 0) NBODY_DEPOSIT_TERM(A, B, 1) NBODY_DEPOSIT_TERM(A, B, 2)
#define NBODY_DEPOSIT_PLANE(A) NBODY_DEPOSIT_ROW(A, 0) NBODY_DEPOSIT_ROW(A, 1) NBODY_DEPOSIT_ROW(A, 2)
    NBODY_DEPOSIT_PLANE(0)
    NBODY_DEPOSIT_PLANE(1)
    NBODY_DEPOSIT_PLANE(2)
#undef NBODY_DEPOSIT_PLANE
#undef NBODY_DEPOSIT_ROW
#undef NBODY_DEPOSIT_TERM
    if constexpr (kLds) {
        __syncthreads();
        for (int k = threadIdx.x; k < kTileSlots; k += kDepositBlock) {
            const int tag = tags[k];
            const unsigned long long v = sums[k];
            if (tag >= 0 && v) global_add(acc, tag, v, issued);
        }
    }
    wave_add(terms, &words->terms);
    wave_add(issued, &words->atomics);
}

__global__ __launch_bounds__(kDepositBlock) void k_deposit_convert(long long* acc, size_t cells, const int* __restrict__ count, int n_upper,
                                                                   const deposit::Words* __restrict__ words) {
    const size_t c = size_t(blockIdx.x) * kDepositBlock + threadIdx.x;
    if (c >= cells) return;
    const int S = deposit::scale_of((unsigned long long)live_count(count, n_upper), __longlong_as_double((long long)words->qmax_bits));
    const double v = deposit::grid_value(acc[c], S);
    acc[c] = __double_as_longlong(v);   // the same eight bytes, read as doubles from here on
}

namespace deposit {

Plan make_plan() {
    const Tuning& t = nbody::tuning();
    Plan p;
    p.sort = t.deposit_sort != 0;
    p.combine = t.deposit_combine != 0;
    p.lds = t.deposit_lds != 0;
    return p;
}

namespace {
int key_bits(size_t cells) {   // the bits of the largest key, `cells` itself
    int b = 1;
    while ((size_t(1) << b) <= cells) ++b;
    return b;
}
size_t sort_tmp_bytes(size_t n_upper, size_t cells) {
    size_t b = 0;
    uint32_t* k = nullptr;
    int* v = nullptr;
    (void)rocprim::radix_sort_pairs(nullptr, b, k, k, v, v, n_upper, 0, unsigned(key_bits(cells)), 0);
    return b;
}
Scratch layout(Carver& c, size_t n_upper, size_t cells, bool with_grid, bool sorted) {
    Scratch w;
    w.words = c.take<Words>(1);
    w.q = c.take<double>(n_upper);
    if (with_grid) w.acc = c.take<long long>(cells);
    if (with_grid && sorted) {
        w.keys = c.take<uint32_t>(2 * n_upper);
        w.rows = c.take<int>(2 * n_upper);
        w.sort_bytes = sort_tmp_bytes(n_upper, cells);
        w.sort_tmp = c.take<char>(w.sort_bytes);
    }
    return w;
}
}  // namespace

size_t scratch_bytes(size_t n_upper, size_t cells, bool with_grid, bool sorted) { Carver c; layout(c, n_upper, cells, with_grid, sorted); return c.offset(); }
Scratch scratch_layout(void* base, size_t n_upper, size_t cells, bool with_grid, bool sorted) {
    Carver c(base);
    return layout(c, n_upper, cells, with_grid, sorted);
}

template <class F>
void launch_q(hipStream_t s, const ShardT<F>& sh, int n_upper, const Grid& g, int quantity, const Scratch& w) {
    (void)hipMemsetAsync(w.words, 0, sizeof(Words), s);
    if (n_upper <= 0) return;
    hipLaunchKernelGGL(k_deposit_q<F>, dim3(blocks_for(n_upper)), dim3(kDepositBlock), 0, s, sh.own_pos(), sh.vel, sh.own_count(), n_upper, g,
                       quantity, w.q, w.words);
}

template <class F>
int launch_deposit(hipStream_t s, const ShardT<F>& sh, int n_upper, const Grid& g, const Plan& p, const Scratch& w, const int* ordered_rows) {
    const size_t cells = cells_of(g);
    (void)hipMemsetAsync(w.acc, 0, cells * sizeof(long long), s);
    if (n_upper > 0) {
        const int* rows = ordered_rows;
        if (p.sort && !ordered_rows) {
            hipLaunchKernelGGL(k_deposit_keys<F>, dim3(blocks_for(n_upper)), dim3(kDepositBlock), 0, s, sh.own_pos(), sh.own_count(), n_upper, g,
                               uint32_t(cells), w.q, w.keys, w.rows);
            size_t tb = w.sort_bytes;
            if (rocprim::radix_sort_pairs(w.sort_tmp, tb, w.keys, w.keys + n_upper, w.rows, w.rows + n_upper, size_t(n_upper), 0,
                                          unsigned(key_bits(cells)), s) != hipSuccess)
                return -1;
            rows = w.rows + n_upper;
        }
        const dim3 grid(blocks_for(n_upper)), block(kDepositBlock);
#define NBODY_DEPOSIT(C, L) \
    hipLaunchKernelGGL((k_deposit<F, C, L>), grid, block, 0, s, sh.own_pos(), sh.own_count(), n_upper, g, w.q, rows, w.words, w.acc)
        if (p.combine && p.lds) NBODY_DEPOSIT(true, true);
        else if (p.combine) NBODY_DEPOSIT(true, false);
        else if (p.lds) NBODY_DEPOSIT(false, true);
        else NBODY_DEPOSIT(false, false);
#undef NBODY_DEPOSIT
    }
    hipLaunchKernelGGL(k_deposit_convert, dim3(unsigned((cells + kDepositBlock - 1) / kDepositBlock)), dim3(kDepositBlock), 0, s, w.acc, cells,
                       sh.own_count(), n_upper, w.words);
    return 0;
}

template void launch_q<float>(hipStream_t, const ShardT<float>&, int, const Grid&, int, const Scratch&);
template void launch_q<double>(hipStream_t, const ShardT<double>&, int, const Grid&, int, const Scratch&);
template int launch_deposit<float>(hipStream_t, const ShardT<float>&, int, const Grid&, const Plan&, const Scratch&, const int*);
template int launch_deposit<double>(hipStream_t, const ShardT<double>&, int, const Grid&, const Plan&, const Scratch&, const int*);

}}  // namespace nbody::deposit
