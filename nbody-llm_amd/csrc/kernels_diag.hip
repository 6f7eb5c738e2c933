// kernels_diag.hip -- whole-state diagnostics of a handle's bodies on the device (gfx950), f64 on either dtype: the ten moment
// sums of nbody_moments and the mass profile of nbody_lagrangian_radii.  Read-only streaming kernels; compiled with
// -ffp-contract=off (every product, sum and difference rounded on its own).  No floating-point atomics anywhere: every sum has
// a fixed association order, so the same input gives the same bits.
//
//   k_diag_moments  one body per lane, ten LDS sums of 256 doubles, k_ext_phi's pairwise tree per block
//   k_diag_keys     r2 = |x - center|^2 as a u64 key (non-negative doubles order as their bit patterns); NaN rows and rows past
//                   the live count get the all-ones key, which sorts behind +inf, and are not counted
//   (rocprim::radix_sort_pairs: stable, so equal r2 keep ascending body index)
//   k_diag_gather   masses into sorted order (0 for the rows left out) and the double-double total of every tile of 256 rows
//   k_diag_scan     inclusive prefix sums of the sorted masses in double-double, rounded to f64 once at the end.  The totals of
//                   the tiles before a tile and the tile's own rows are added in patterns that depend on the tile index alone
//                   (rocPRIM's decoupled look-back scan groups the earlier tiles by their completion order, and neither f64 nor
//                   double-double addition is associative: kernels_tree.hip has the story)
//   k_diag_radii    one lane per fraction: binary search over the prefixes, sqrt of the key found
#include "kernels_diag.h"
#include "real.h"   // widen
#include "scratch_carve.h"

#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>

namespace nbody {

using diag::kDiagBlock;
using diag::kMoments;

namespace {

constexpr unsigned long long kLeftOut = ~0ull;   // (a NaN's bit pattern: no r2 that is kept has it)

// s + e = a + b exactly (Knuth; no assumption on the sizes)
__device__ __forceinline__ void two_sum(double a, double b, double& s, double& e) {
    s = a + b;
    const double bb = s - a;
    e = (a - (s - bb)) + (b - bb);
}
// the same for |a| >= |b| (Dekker)
__device__ __forceinline__ void fast_two_sum(double a, double b, double& s, double& e) {
    s = a + b;
    e = b - (s - a);
}
struct DD { double hi, lo; };   // hi + lo, |lo| <= ulp(hi) / 2
// (a.hi + a.lo) + (b.hi + b.lo), the accurate variant of kernels_tree.hip's dd_add: a few 2^-106 of |a + b|
__device__ __forceinline__ DD dd_add(const DD a, const DD b) {
    double s, e, t, f;
    two_sum(a.hi, b.hi, s, e);
    two_sum(a.lo, b.lo, t, f);
    e += t;
    fast_two_sum(s, e, s, e);
    e += f;
    DD r;
    fast_two_sum(s, e, r.hi, r.lo);
    return r;
}

// sum over the block's kDiagBlock values, pairwise: hi[t] += hi[t + half] for half = 128 ... 1 in double-double.  Every thread
// calls it; the total is in (hi[0], lo[0]) afterwards.
__device__ __forceinline__ void dd_block_sum(double* hi, double* lo, int t) {
    __syncthreads();
    for (int half = kDiagBlock / 2; half > 0; half >>= 1) {
        if (t < half) {
            const DD r = dd_add(DD{hi[t], lo[t]}, DD{hi[t + half], lo[t + half]});
            hi[t] = r.hi;
            lo[t] = r.lo;
        }
        __syncthreads();
    }
}

}  // namespace

template <class F>
__global__ __launch_bounds__(kDiagBlock) void k_diag_moments(const typename Real<F>::V4* __restrict__ pos,
                                                             const typename Real<F>::V4* __restrict__ vel,
                                                             const int* __restrict__ count, double* __restrict__ part) {
    __shared__ double sum[kMoments][kDiagBlock];
    const int t = threadIdx.x;
    const int k = blockIdx.x * kDiagBlock + t;
    double term[kMoments] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (k < *count) {
        const double4 p = widen(pos[k]);
        const double4 v = widen(vel[k]);
        const double m = p.w;
        term[0] = m;
        term[1] = m * p.x;
        term[2] = m * p.y;
        term[3] = m * p.z;
        term[4] = m * v.x;
        term[5] = m * v.y;
        term[6] = m * v.z;
        term[7] = (p.y * v.z - p.z * v.y) * m;
        term[8] = (p.z * v.x - p.x * v.z) * m;
        term[9] = (p.x * v.y - p.y * v.x) * m;
    }
#pragma unroll
    for (int q = 0; q < kMoments; ++q) sum[q][t] = term[q];
    __syncthreads();
    for (int half = kDiagBlock / 2; half > 0; half >>= 1) {   // sum[t] += sum[t + half]: the same pairs whatever the schedule
        if (t < half) {
#pragma unroll
            for (int q = 0; q < kMoments; ++q) sum[q][t] = sum[q][t] + sum[q][t + half];
        }
        __syncthreads();
    }
    if (t < kMoments) part[size_t(blockIdx.x) * kMoments + t] = sum[t][0];
}

template <class F>
__global__ __launch_bounds__(kDiagBlock) void k_diag_keys(const typename Real<F>::V4* __restrict__ pos, const int* __restrict__ count,
                                                          int n_upper, const double* __restrict__ center,
                                                          unsigned long long* __restrict__ keys, int* __restrict__ idx,
                                                          int* __restrict__ n_valid) {
    const int k = blockIdx.x * kDiagBlock + threadIdx.x;
    unsigned long long key = kLeftOut;
    if (k < n_upper && k < *count) {
        const double4 p = widen(pos[k]);
        const double dx = p.x - center[0], dy = p.y - center[1], dz = p.z - center[2];
        const double r2 = (dx * dx + dy * dy) + dz * dz;
        if (r2 == r2) key = (unsigned long long)__double_as_longlong(r2);
    }
    if (k < n_upper) { keys[k] = key; idx[k] = k; }
    const int valid = __syncthreads_count(key != kLeftOut);
    if (threadIdx.x == 0 && valid) atomicAdd(n_valid, valid);   // (an integer count: the order of the additions does not matter)
}

template <class F>
__global__ __launch_bounds__(kDiagBlock) void k_diag_gather(const typename Real<F>::V4* __restrict__ pos,
                                                            const unsigned long long* __restrict__ keys, const int* __restrict__ idx,
                                                            int n_upper, double* __restrict__ m_sorted, double* __restrict__ tot_hi,
                                                            double* __restrict__ tot_lo) {
    __shared__ double hi[kDiagBlock], lo[kDiagBlock];
    const int t = threadIdx.x;
    const int k = blockIdx.x * kDiagBlock + t;
    double m = 0.0;
    if (k < n_upper) {
        if (keys[k] != kLeftOut) m = double(pos[idx[k]].w);
        m_sorted[k] = m;
    }
    hi[t] = m;
    lo[t] = 0.0;
    dd_block_sum(hi, lo, t);
    if (t == 0) { tot_hi[blockIdx.x] = hi[0]; tot_lo[blockIdx.x] = lo[0]; }
}

__global__ __launch_bounds__(kDiagBlock) void k_diag_scan(int n_upper, const double* __restrict__ tot_hi, const double* __restrict__ tot_lo,
                                                          double* __restrict__ c /* in: sorted masses; out: inclusive prefixes */) {
    __shared__ double hi[kDiagBlock], lo[kDiagBlock];
    const int t = threadIdx.x;
    const int k = blockIdx.x * kDiagBlock + t;
    // the tiles before this one: lane t adds its run of consecutive tiles in ascending order, the block adds the 256 runs pairwise
    const int before = int(blockIdx.x);
    const int per = (before + kDiagBlock - 1) / kDiagBlock;
    DD run{0.0, 0.0};
    for (int q = 0; q < per; ++q) {
        const int b = t * per + q;
        if (b < before) run = dd_add(run, DD{tot_hi[b], tot_lo[b]});
    }
    hi[t] = run.hi;
    lo[t] = run.lo;
    dd_block_sum(hi, lo, t);
    const DD carry{hi[0], lo[0]};
    __syncthreads();
    // the tile's own rows: a Hillis-Steele scan in LDS, v[t] = v[t - off] + v[t] for off = 1 ... 128
    DD v{k < n_upper ? c[k] : 0.0, 0.0};
    hi[t] = v.hi;
    lo[t] = v.lo;
    __syncthreads();
    for (int off = 1; off < kDiagBlock; off <<= 1) {
        DD left{0.0, 0.0};
        if (t >= off) left = DD{hi[t - off], lo[t - off]};
        __syncthreads();
        if (t >= off) {
            v = dd_add(left, v);
            hi[t] = v.hi;
            lo[t] = v.lo;
        }
        __syncthreads();
    }
    if (k < n_upper) c[k] = dd_add(carry, v).hi;   // (hi of a normalised pair is the double nearest to it)
}

__global__ __launch_bounds__(kDiagBlock) void k_diag_radii(const unsigned long long* __restrict__ keys, const double* __restrict__ c,
                                                           const int* __restrict__ n_valid, const double* __restrict__ fractions,
                                                           int n_frac, double* __restrict__ out) {
    const int k = blockIdx.x * kDiagBlock + threadIdx.x;
    const int nv = *n_valid;
    const double mass = nv > 0 ? c[nv - 1] : 0.0;
    if (k == 0) out[n_frac] = mass;
    if (k >= n_frac) return;
    double radius = __longlong_as_double(0x7ff8000000000000ll);   // NaN: no body in the order, or none whose prefix reaches the target
    if (nv > 0) {
        const double target = fractions[k] * mass;
        int lo = 0, hi = nv - 1;   // the first j with c[j] >= target, if c[nv - 1] is one
        if (c[hi] >= target) {
            while (lo < hi) {
                const int mid = lo + (hi - lo) / 2;
                if (c[mid] >= target) hi = mid; else lo = mid + 1;
            }
            radius = __builtin_sqrt(__longlong_as_double((long long)keys[lo]));
        }
    }
    out[k] = radius;
}

namespace diag {

template <class F>
void launch_diag_moments(hipStream_t s, const ShardT<F>& sh, int n_upper, double* part) {
    const int blocks = blocks_for(n_upper);
    if (blocks == 0) return;
    hipLaunchKernelGGL(k_diag_moments<F>, dim3(blocks), dim3(kDiagBlock), 0, s, sh.own_pos(), sh.vel, sh.own_count(), part);
}

namespace {
size_t sort_tmp_bytes(size_t n_upper) {
    size_t b = 0;
    unsigned long long* k = nullptr;
    int* v = nullptr;
    (void)rocprim::radix_sort_pairs(nullptr, b, k, k, v, v, n_upper, 0, 64, 0);
    return b;
}
RadiiScratch layout(Carver& c, size_t n_upper, size_t n_frac) {
    const size_t tiles = size_t(blocks_for(int(n_upper)));
    RadiiScratch w;
    w.keys = c.take<unsigned long long>(2 * n_upper);
    w.idx = c.take<int>(2 * n_upper);
    w.c = c.take<double>(n_upper);
    w.totals = c.take<double>(2 * tiles);
    w.n_valid = c.take<int>(1);
    w.center = c.take<double>(3);
    w.fractions = c.take<double>(n_frac);
    w.out = c.take<double>(n_frac + 1);
    w.sort_bytes = sort_tmp_bytes(n_upper);
    w.sort_tmp = c.take<char>(w.sort_bytes);
    return w;
}
}  // namespace

size_t radii_scratch_bytes(size_t n_upper, size_t n_frac) { Carver c; layout(c, n_upper, n_frac); return c.offset(); }
RadiiScratch radii_scratch_layout(void* base, size_t n_upper, size_t n_frac) { Carver c(base); return layout(c, n_upper, n_frac); }

template <class F>
int launch_diag_radii(hipStream_t s, const ShardT<F>& sh, int n_upper, int n_frac, const RadiiScratch& w) {
    const int blocks = blocks_for(n_upper);
    if (blocks == 0) return 0;
    const size_t n = size_t(n_upper);
    if (hipMemsetAsync(w.n_valid, 0, sizeof(int), s) != hipSuccess) return -1;
    hipLaunchKernelGGL(k_diag_keys<F>, dim3(blocks), dim3(kDiagBlock), 0, s, sh.own_pos(), sh.own_count(), n_upper, w.center, w.keys, w.idx,
                       w.n_valid);
    size_t tb = w.sort_bytes;
    if (rocprim::radix_sort_pairs(w.sort_tmp, tb, w.keys, w.keys + n, w.idx, w.idx + n, n, 0, 64, s) != hipSuccess) return -1;
    hipLaunchKernelGGL(k_diag_gather<F>, dim3(blocks), dim3(kDiagBlock), 0, s, sh.own_pos(), w.keys + n, w.idx + n, n_upper, w.c, w.totals,
                       w.totals + blocks);
    hipLaunchKernelGGL(k_diag_scan, dim3(blocks), dim3(kDiagBlock), 0, s, n_upper, w.totals, w.totals + blocks, w.c);
    hipLaunchKernelGGL(k_diag_radii, dim3(std::max(1, blocks_for(n_frac))), dim3(kDiagBlock), 0, s, w.keys + n, w.c, w.n_valid, w.fractions,
                       n_frac, w.out);
    return 0;
}

template void launch_diag_moments<float>(hipStream_t, const ShardT<float>&, int, double*);
template void launch_diag_moments<double>(hipStream_t, const ShardT<double>&, int, double*);
template int launch_diag_radii<float>(hipStream_t, const ShardT<float>&, int, int, const RadiiScratch&);
template int launch_diag_radii<double>(hipStream_t, const ShardT<double>&, int, int, const RadiiScratch&);

}}  // namespace nbody::diag
